// chordal.hip — kmx_chordal_*: chordal initialisation of a batch of pose
// graphs on the device (the problem kmx.dpgo.init's
// chordal_initialization solves on the host).
//
// Poses are cut into blocks (a robot each); both ends of an edge lie in one
// block; anchors are held at R = I, t = 0. Stage 1 solves the connection
// Laplacian for the unconstrained 3x3 blocks (three right-hand sides, the rows
// of X), k_ch_project takes every free block to SO(3), stage 2 solves the
// scalar graph Laplacian for the translations (three right-hand sides, the
// components of t). Both stages are Jacobi-preconditioned CG, ONE CG PER
// (block, row): alpha, beta, the stop test and the iteration count are per
// (block, row) and live on the device (ChScal).
//
// Sums are ordered. A pose adds its incident edges in the CSR's order; a tile
// (at most 64 consecutive poses of one block, one wave) reduces with a fixed
// shuffle tree; a block's tile partials are summed by one wave in a fixed
// order (k_ch_reduce). No atomics on floating-point data: the only atomic is
// the integer count of (block, row) pairs still running, which every launch
// tests so that a launch enqueued past convergence returns at once. The host
// enqueues check_every iterations at a time and reads that count in between;
// a (block, row) stops itself at max_iterations, so the result does not depend
// on check_every. No grid barrier, no persistent kernel, no device-side wait.
//
// kmx_chordal_solve_robust wraps the two stages in GNC-TLS: after each solve
// k_ch_gnc forms every edge's residual and factor g for its block's mu and the
// next solve's weights w0 g, k_ch_decide keeps mu, the update count and the
// stop test per block on the device, and a block that is done is frozen (its
// CGs do not start, it is not projected again, its weights are not rewritten),
// so the batch still changes no bit of a block's result.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "chordal_host.h"
#include "common.h"
#include "so3_project.h"

namespace {
using kmx::CH_TILE;

// One CG's scalars: a (block, row) of one stage.
struct ChScal {
  double bb, rr, rz, alpha, beta;
  int active, iters, conv, pad;
};

// One block's GNC state (kmx_chordal_solve_robust); all of it lives on the device.
struct ChRob {
  double mu;       // the mu the block's current g was formed with
  double mu_next;  // the mu the next GNC pass uses
  int updates, done, conv;
  int n1, n0, nf;          // edges at g = 1, g = 0, in between (not fixed, w0 > 0)
  int it_rot, it_trans;    // CG iterations, summed over the block's solves
};

constexpr int CH_NPART = 9;  // partial sums per tile: up to 3 quantities x 3 rows

using kmx::wave_sum;  // lane 0 holds the sum; fixed tree

struct ChTiles {
  const int *p0, *p1, *block;
};

struct ChInc {
  const int* ptr;
  const uint32_t* other;
  const double* w;  // w*kappa (rotations) or w*tau (translations); 0: the edge is dropped
  const double* M;  // [rec][9]
};

// out_p = D_p in_p - sum_rec w in_other M (W = 3: rows of 3, M = R_e or R_e^T;
// W = 1: M = 1) for the free poses of a tile.
//   INIT: in = the start vector with the anchors' values in place; writes the
//         residual r = rhs - out (rhs: the translations' right-hand side, or 0
//         for the rotations, whose right-hand side is the anchors' terms
//         inside out) and d = z = r / D, and the partials <b,b>, <r,r>, <r,z>.
//   else: in = d; writes q = out for the rows still running and the partials
//         <d, q>.
template <int W, bool INIT>
__global__ __launch_bounds__(CH_TILE) void k_ch_apply(ChTiles T, ChInc I, const uint8_t* __restrict__ is_free,
                                                      const double* __restrict__ D, const double* __restrict__ in,
                                                      const double* __restrict__ rhs, double* __restrict__ out,
                                                      double* __restrict__ dvec, const ChScal* __restrict__ sc,
                                                      const int* __restrict__ n_active, double* __restrict__ part,
                                                      const ChRob* __restrict__ rb) {
  constexpr int V = 3 * W;
  if (!INIT && *n_active == 0) return;
  const int tile = blockIdx.x, b = T.block[tile];
  if (INIT && rb && rb[b].done) return;  // a frozen block of the robust solve: its CGs do not start
  bool act[3] = {true, true, true};
  if (!INIT) {
    for (int a = 0; a < 3; ++a) act[a] = sc[3 * b + a].active != 0;
    if (!act[0] && !act[1] && !act[2]) return;
  }
  const int p = T.p0[tile] + (int)threadIdx.x;
  const bool in_tile = p < T.p1[tile];
  const bool valid = in_tile && is_free[p];
  double acc[V], banc[V], x[V];
  for (int k = 0; k < V; ++k) acc[k] = banc[k] = x[k] = 0.0;
  if (valid) {
    const double Dp = D[p];
    for (int k = 0; k < V; ++k) {
      x[k] = in[(size_t)V * p + k];
      acc[k] = Dp * x[k];
    }
    const int k1 = I.ptr[p + 1];
    for (int k = I.ptr[p]; k < k1; ++k) {
      const double w = I.w[k];
      if (w == 0.0) continue;
      const int o = (int)(I.other[k] & 0x7fffffffu);
      double xo[V];
      for (int c = 0; c < V; ++c) xo[c] = in[(size_t)V * o + c];
      if (W == 3) {
        double M[9];
        for (int c = 0; c < 9; ++c) M[c] = I.M[(size_t)9 * k + c];
        const bool anc = INIT && !is_free[o];
        for (int a = 0; a < 3; ++a)
          for (int c = 0; c < 3; ++c) {
            const double v = w * (xo[3 * a] * M[c] + xo[3 * a + 1] * M[3 + c] + xo[3 * a + 2] * M[6 + c]);
            acc[3 * a + c] -= v;
            if (anc) banc[3 * a + c] += v;
          }
      } else {
        for (int a = 0; a < 3; ++a) acc[a] -= w * xo[a];
      }
    }
  }
  if (INIT) {
    double s[CH_NPART];
    for (int k = 0; k < CH_NPART; ++k) s[k] = 0.0;
    if (in_tile) {
      const double Dp = valid ? D[p] : 1.0;
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < W; ++c) {
          const int k = W * a + c;
          const double bv = valid ? (W == 3 ? banc[k] : rhs[(size_t)V * p + k]) : 0.0;
          const double r = valid ? (W == 3 ? -acc[k] : bv - acc[k]) : 0.0;
          const double z = r / Dp;
          out[(size_t)V * p + k] = r;
          dvec[(size_t)V * p + k] = z;
          s[a] += bv * bv;
          s[3 + a] += r * r;
          s[6 + a] += r * z;
        }
    }
    for (int k = 0; k < CH_NPART; ++k) {
      const double v = wave_sum(s[k]);
      if (threadIdx.x == 0) part[(size_t)CH_NPART * tile + k] = v;
    }
  } else {
    double s[3] = {0.0, 0.0, 0.0};
    if (valid)
      for (int a = 0; a < 3; ++a)
        if (act[a])
          for (int c = 0; c < W; ++c) {
            const int k = W * a + c;
            out[(size_t)V * p + k] = acc[k];
            s[a] += x[k] * acc[k];
          }
    for (int a = 0; a < 3; ++a) {
      const double v = wave_sum(s[a]);
      if (threadIdx.x == 0) part[(size_t)CH_NPART * tile + a] = v;
    }
  }
}

// A block's tile partials, summed by one wave in a fixed order (lane l takes
// tiles l, l + 64, ... in turn, then the shuffle tree), and the decision.
//   PHASE 0: <b,b>, <r,r>, <r,z> of the start: who runs at all
//   PHASE 1: <d,q>: alpha
//   PHASE 2: <r,r>, <r,z> after the update: beta, the stop test, the count
template <int PHASE>
__global__ __launch_bounds__(64) void k_ch_reduce(const int* __restrict__ tile_ptr, const double* __restrict__ part,
                                                  ChScal* __restrict__ sc, int* __restrict__ n_active, double rtol2,
                                                  int max_it, const ChRob* __restrict__ rb) {
  if (PHASE != 0 && *n_active == 0) return;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (PHASE == 0 && rb && rb[b].done) return;  // frozen: its scalars stay those of its last solve (active = 0)
  const int t0 = tile_ptr[b], t1 = tile_ptr[b + 1];
  constexpr int NQ = PHASE == 0 ? 3 : PHASE == 1 ? 1 : 2;
  for (int a = 0; a < 3; ++a) {
    ChScal* s = sc + 3 * b + a;
    if (PHASE != 0 && !s->active) continue;  // the same for the whole wave
    double v[NQ];
    for (int q = 0; q < NQ; ++q) {
      double u = 0.0;
      for (int t = t0 + lane; t < t1; t += 64) u += part[(size_t)CH_NPART * t + 3 * q + a];
      v[q] = wave_sum(u);
    }
    if (lane != 0) continue;
    if (PHASE == 0) {
      const bool conv = v[0] == 0.0 || v[1] <= rtol2 * v[0];
      s->bb = v[0];
      s->rr = v[1];
      s->rz = v[2];
      s->alpha = s->beta = 0.0;
      s->iters = 0;
      s->conv = conv;
      s->active = !conv && max_it > 0;
      s->pad = 0;
      if (s->active) atomicAdd(n_active, 1);
    } else if (PHASE == 1) {
      if (v[0] > 0.0) {
        s->alpha = s->rz / v[0];
      } else {  // H is positive definite: d = 0 or a NaN; stop this one, not converged
        s->active = 0;
        atomicSub(n_active, 1);
      }
    } else {
      s->iters += 1;
      s->beta = v[1] / s->rz;
      s->rz = v[1];
      s->rr = v[0];
      if (v[0] <= rtol2 * s->bb) {
        s->conv = 1;
        s->active = 0;
        atomicSub(n_active, 1);
      } else if (s->iters >= max_it) {
        s->active = 0;
        atomicSub(n_active, 1);
      }
    }
  }
}

// x += alpha d, r -= alpha q for the rows still running; partials <r,r>, <r,z>.
template <int W>
__global__ __launch_bounds__(CH_TILE) void k_ch_update(ChTiles T, const uint8_t* __restrict__ is_free,
                                                       const double* __restrict__ D, double* __restrict__ x,
                                                       double* __restrict__ r, const double* __restrict__ d,
                                                       const double* __restrict__ q, const ChScal* __restrict__ sc,
                                                       const int* __restrict__ n_active, double* __restrict__ part) {
  constexpr int V = 3 * W;
  if (*n_active == 0) return;
  const int tile = blockIdx.x, b = T.block[tile];
  bool act[3];
  double alpha[3];
  for (int a = 0; a < 3; ++a) {
    act[a] = sc[3 * b + a].active != 0;
    alpha[a] = sc[3 * b + a].alpha;
  }
  if (!act[0] && !act[1] && !act[2]) return;
  const int p = T.p0[tile] + (int)threadIdx.x;
  const bool valid = p < T.p1[tile] && is_free[p];
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (valid) {
    const double Dp = D[p];
    for (int a = 0; a < 3; ++a)
      if (act[a])
        for (int c = 0; c < W; ++c) {
          const size_t k = (size_t)V * p + W * a + c;
          x[k] += alpha[a] * d[k];
          const double rn = r[k] - alpha[a] * q[k];
          r[k] = rn;
          s[a] += rn * rn;
          s[3 + a] += rn * (rn / Dp);
        }
  }
  for (int k = 0; k < 6; ++k) {
    const double v = wave_sum(s[k]);
    if (threadIdx.x == 0) part[(size_t)CH_NPART * tile + k] = v;
  }
}

// d = z + beta d with z = r / D, for the rows that go on.
template <int W>
__global__ __launch_bounds__(CH_TILE) void k_ch_dir(ChTiles T, const uint8_t* __restrict__ is_free,
                                                    const double* __restrict__ D, const double* __restrict__ r,
                                                    double* __restrict__ d, const ChScal* __restrict__ sc,
                                                    const int* __restrict__ n_active) {
  constexpr int V = 3 * W;
  if (*n_active == 0) return;
  const int tile = blockIdx.x, b = T.block[tile];
  const int p = T.p0[tile] + (int)threadIdx.x;
  if (p >= T.p1[tile] || !is_free[p]) return;
  const double Dp = D[p];
  for (int a = 0; a < 3; ++a) {
    if (!sc[3 * b + a].active) continue;
    const double beta = sc[3 * b + a].beta;
    for (int c = 0; c < W; ++c) {
      const size_t k = (size_t)V * p + W * a + c;
      d[k] = r[k] / Dp + beta * d[k];
    }
  }
}

// D_p of both stages: the sums of w*kappa and of w*tau over a pose's records.
__global__ void k_ch_diag(int n, const int* __restrict__ inc_ptr, const double* __restrict__ wk,
                          const double* __restrict__ wt, double* __restrict__ Dk, double* __restrict__ Dt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  double a = 0.0, b = 0.0;
  for (int k = inc_ptr[p]; k < inc_ptr[p + 1]; ++k) {
    a += wk[k];
    b += wt[k];
  }
  Dk[p] = a;
  Dt[p] = b;
}

// The translations' right-hand side from the projected rotations:
// b_p = sum_{e: p=j} w tau R_i t_ij - sum_{e: p=i} w tau R_p t_ij; 0 at anchors.
__global__ void k_ch_rhs_t(int n, const int* __restrict__ inc_ptr, const uint32_t* __restrict__ inc_other,
                           const double* __restrict__ wt, const double* __restrict__ inc_t,
                           const uint8_t* __restrict__ is_free, const double* __restrict__ Rv,
                           double* __restrict__ bt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  double b[3] = {0.0, 0.0, 0.0};
  if (is_free[p])
    for (int k = inc_ptr[p]; k < inc_ptr[p + 1]; ++k) {
      const double w = wt[k];
      if (w == 0.0) continue;
      const uint32_t rec = inc_other[k];
      const bool outgoing = (rec & kmx::CH_DIR_OUT) != 0;
      const int i = outgoing ? p : (int)(rec & 0x7fffffffu);
      const double s = outgoing ? -w : w;
      const double* R = Rv + (size_t)9 * i;
      const double* t = inc_t + (size_t)3 * k;
      for (int c = 0; c < 3; ++c) b[c] += s * (R[3 * c] * t[0] + R[3 * c + 1] * t[1] + R[3 * c + 2] * t[2]);
    }
  for (int c = 0; c < 3; ++c) bt[(size_t)3 * p + c] = b[c];
}

// The nearest rotation to every free 3x3 block (so3_project.h).
__global__ void k_ch_project(int n, const uint8_t* __restrict__ is_free, double* __restrict__ X) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !is_free[p]) return;
  double Rm[3][3];
  kmx::so3_project_block(X + (size_t)9 * p, Rm);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) X[(size_t)9 * p + 3 * r + c] = Rm[r][c];
}

// The robust solve's projection, over the tiles: the blocks that are done are
// left alone. Xu holds the unprojected iterate (the next update's start
// vector), X gets the rotations; with keep_projected Xu gets them too.
__global__ __launch_bounds__(CH_TILE) void k_ch_project_tiles(ChTiles T, const ChRob* __restrict__ rb,
                                                              const uint8_t* __restrict__ is_free,
                                                              double* __restrict__ Xu, double* __restrict__ X,
                                                              int keep_projected) {
  const int tile = blockIdx.x;
  if (rb[T.block[tile]].done) return;
  const int p = T.p0[tile] + (int)threadIdx.x;
  if (p >= T.p1[tile] || !is_free[p]) return;
  double Rm[3][3];
  kmx::so3_project_block(Xu + (size_t)9 * p, Rm);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      X[(size_t)9 * p + 3 * r + c] = Rm[r][c];
      if (keep_projected) Xu[(size_t)9 * p + 3 * r + c] = Rm[r][c];
    }
}

// ---- GNC-TLS around the two solves (kmx_chordal_solve_robust)
//
// The arithmetic that decides an edge's weight is stated without contraction:
// both records of an edge, every instantiation of the pass and
// kmx_chordal_residuals must give the same bits.

// r^2 = kappa |R_j - R_i R_ij|_F^2 + tau |t_j - t_i - R_i t_ij|^2
__device__ __forceinline__ double ch_edge_r2(const double* Ri, const double* ti, const double* Rj, const double* tj,
                                             const double* Rij, const double* tij, double kappa, double tau) {
#pragma clang fp contract(off)
  double sr = 0.0, st = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) {
      double v = Ri[3 * a] * Rij[c];
      v += Ri[3 * a + 1] * Rij[3 + c];
      v += Ri[3 * a + 2] * Rij[6 + c];
      const double e = Rj[3 * a + c] - v;
      sr += e * e;
    }
  for (int c = 0; c < 3; ++c) {
    double v = Ri[3 * c] * tij[0];
    v += Ri[3 * c + 1] * tij[1];
    v += Ri[3 * c + 2] * tij[2];
    const double e = (tj[c] - ti[c]) - v;
    st += e * e;
  }
  return kappa * sr + tau * st;
}

// The TLS factor; *cls: 1 (g = 1), 0 (g = 0), 2 (in between).
__device__ __forceinline__ double ch_tls(double r2, double mu, double c2, int* cls) {
#pragma clang fp contract(off)
  const double lo = mu / (mu + 1.0) * c2, hi = (mu + 1.0) / mu * c2;
  if (r2 <= lo) {
    *cls = 1;
    return 1.0;
  }
  if (r2 >= hi) {
    *cls = 0;
    return 0.0;
  }
  *cls = 2;
  return sqrt(c2 * mu * (mu + 1.0) / r2) - mu;
}

struct ChGnc {  // per incidence record
  const int* ptr;
  const uint32_t* other;
  const double *M, *t, *kappa, *tau, *w0;
  const uint8_t* fixed;
};

// The GNC pass: a lane per pose over the tiles. A lane walks its records in
// CSR order and evaluates each edge in its canonical i -> j orientation (at
// the source's record R_ij is the stored M transposed: an index swap), so an
// edge's two records get the same bits, and writes only its own records and
// its own D_p. An edge is counted once, at its target's record.
//   MODE 0: after the first solve: g = 1 everywhere, the tile's largest r^2
//           and the number of counted edges (not fixed, w0 > 0)
//   MODE 1: g for the block's mu_next, the records' w0 g kappa / w0 g tau and
//           D_p of both stages; per tile the counts of g = 1, g = 0, in
//           between, and of edges whose g differs from the one in place
//   MODE 2: kmx_chordal_residuals: r^2 to wk and, with mu_in, g to wt
template <int MODE>
__global__ __launch_bounds__(CH_TILE) void k_ch_gnc(ChTiles T, ChGnc G, const double* __restrict__ Rv,
                                                    const double* __restrict__ tv, const ChRob* __restrict__ rb,
                                                    const double* __restrict__ mu_in, double c2,
                                                    double* __restrict__ rg, double* __restrict__ wk,
                                                    double* __restrict__ wt, double* __restrict__ Dk,
                                                    double* __restrict__ Dt, double* __restrict__ pmax,
                                                    int* __restrict__ pcnt) {
  const int tile = blockIdx.x, b = T.block[tile];
  if (MODE != 2 && rb[b].done) return;
  const double mu = MODE == 1 ? rb[b].mu_next : (MODE == 2 && mu_in) ? mu_in[b] : 0.0;
  const int p = T.p0[tile] + (int)threadIdx.x;
  double mx = 0.0;
  int n1 = 0, n0 = 0, nf = 0, nch = 0;
  if (p < T.p1[tile]) {
    double Rp[9], tp[3], dk = 0.0, dt = 0.0;
    for (int c = 0; c < 9; ++c) Rp[c] = Rv[(size_t)9 * p + c];
    for (int c = 0; c < 3; ++c) tp[c] = tv[(size_t)3 * p + c];
    const int k1 = G.ptr[p + 1];
    for (int k = G.ptr[p]; k < k1; ++k) {
      const uint32_t rec = G.other[k];
      const bool outgoing = (rec & kmx::CH_DIR_OUT) != 0;
      const int o = (int)(rec & 0x7fffffffu);
      double Ri[9], Rj[9], Rij[9], ti[3], tj[3], tij[3];
      for (int c = 0; c < 9; ++c) {
        const double ro = Rv[(size_t)9 * o + c];
        Ri[c] = outgoing ? Rp[c] : ro;
        Rj[c] = outgoing ? ro : Rp[c];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          const double m_rc = G.M[(size_t)9 * k + 3 * r + c], m_cr = G.M[(size_t)9 * k + 3 * c + r];
          Rij[3 * r + c] = outgoing ? m_cr : m_rc;
        }
      for (int c = 0; c < 3; ++c) {
        const double to = tv[(size_t)3 * o + c];
        ti[c] = outgoing ? tp[c] : to;
        tj[c] = outgoing ? to : tp[c];
        tij[c] = G.t[(size_t)3 * k + c];
      }
      const double r2 = ch_edge_r2(Ri, ti, Rj, tj, Rij, tij, G.kappa[k], G.tau[k]);
      const bool fixed = G.fixed[k] != 0;
      const double w0 = G.w0[k];
      const bool counted = !fixed && w0 > 0.0 && !outgoing;
      if (MODE == 0) {
        rg[k] = 1.0;
        if (counted) {
          mx = fmax(mx, r2);
          ++n1;
        }
      } else if (MODE == 1) {
        int cls = 1;
        const double g = fixed ? 1.0 : ch_tls(r2, mu, c2, &cls);
        if (counted) {
          n1 += cls == 1;
          n0 += cls == 0;
          nf += cls == 2;
          nch += g != rg[k];
        }
        rg[k] = g;
        const double w = w0 * g, a = w * G.kappa[k], c = w * G.tau[k];
        wk[k] = a;
        wt[k] = c;
        dk += a;
        dt += c;
      } else {
        wk[k] = r2;
        if (mu_in) {
          int cls;
          wt[k] = fixed ? 1.0 : ch_tls(r2, mu, c2, &cls);
        }
      }
    }
    if (MODE == 1) {
      Dk[p] = dk;
      Dt[p] = dt;
    }
  }
  if (MODE == 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off, 64));
    n1 = wave_sum(n1);
    if (threadIdx.x == 0) {
      pmax[tile] = mx;
      pcnt[4 * tile] = n1;
    }
  } else if (MODE == 1) {
    n1 = wave_sum(n1);
    n0 = wave_sum(n0);
    nf = wave_sum(nf);
    nch = wave_sum(nch);
    if (threadIdx.x == 0) {
      pcnt[4 * tile] = n1;
      pcnt[4 * tile + 1] = n0;
      pcnt[4 * tile + 2] = nf;
      pcnt[4 * tile + 3] = nch;
    }
  }
}

// A block's decision, one wave per block over its tile partials (a max and
// integer sums: exact in any order, and taken in a fixed one).
//   FIRST: after the first solve and k_ch_gnc<0>: mu_0, or done with 0 updates
//   else:  account (a solve was run since the last decision): its update and
//          iterations are counted; last: the block stops here, not converged,
//          and keeps the g of that solve; otherwise, after k_ch_gnc<1>: the
//          stop test on the new g, or mu_next <- mu mu_step
template <bool FIRST>
__global__ __launch_bounds__(64) void k_ch_decide(const int* __restrict__ tile_ptr, const double* __restrict__ pmax,
                                                  const int* __restrict__ pcnt, ChRob* __restrict__ rb,
                                                  const ChScal* __restrict__ sc, int nb, int* __restrict__ n_running,
                                                  double c2, double mu_init, double mu_step, int account, int last) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  ChRob* s = rb + b;
  if (!FIRST && s->done) return;  // the same for the whole wave
  const int t0 = tile_ptr[b], t1 = tile_ptr[b + 1];
  int it_rot = 0, it_trans = 0;
  for (int a = 0; a < 3; ++a) {
    it_rot = max(it_rot, sc[3 * b + a].iters);
    it_trans = max(it_trans, sc[3 * nb + 3 * b + a].iters);
  }
  if (FIRST) {
    double mx = 0.0;
    int n1 = 0;
    for (int t = t0 + lane; t < t1; t += 64) {
      mx = fmax(mx, pmax[t]);
      n1 += pcnt[4 * t];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off, 64));
    n1 = wave_sum(n1);
    if (lane != 0) return;
    s->mu = 0.0;
    s->mu_next = 0.0;
    s->updates = 0;
    s->done = 0;
    s->conv = 0;
    s->n1 = n1;
    s->n0 = s->nf = 0;
    s->it_rot = it_rot;
    s->it_trans = it_trans;
    const double two_mx = 2.0 * mx;
    if (mu_init > 0.0) {
      s->mu_next = mu_init;
    } else if (two_mx <= c2) {
      s->done = 1;
      s->conv = 1;
    } else {
      s->mu_next = c2 / (two_mx - c2);
    }
    if (!s->done) atomicAdd(n_running, 1);
  } else {
    int cnt[4] = {0, 0, 0, 0};
    if (!last) {
      for (int t = t0 + lane; t < t1; t += 64)
        for (int q = 0; q < 4; ++q) cnt[q] += pcnt[4 * t + q];
      for (int q = 0; q < 4; ++q) cnt[q] = wave_sum(cnt[q]);
    }
    if (lane != 0) return;
    if (account) {
      s->updates += 1;
      s->it_rot += it_rot;
      s->it_trans += it_trans;
    }
    if (last) {
      s->done = 1;
      atomicSub(n_running, 1);
      return;
    }
    s->mu = s->mu_next;
    s->n1 = cnt[0];
    s->n0 = cnt[1];
    s->nf = cnt[2];
    if (cnt[2] == 0 && cnt[3] == 0) {  // every g is 0 or 1 and none changed: the last solve is the answer
      s->done = 1;
      s->conv = 1;
      atomicSub(n_running, 1);
    } else {
      s->mu_next = s->mu * mu_step;
    }
  }
}

// The robust solve's arrays: allocated as a whole by its first call after
// set_graph (ch_robust_reserve), freed with the graph.
struct ChRobDev {
  kmx::DevBuf<double> rkappa, rtau, rw0;  // [2m] per record
  kmx::DevBuf<uint8_t> rfixed;            // [2m]
  kmx::DevBuf<double> rg, gwk, gwt;       // [2m] g and the records' w0 g kappa / w0 g tau
  kmx::DevBuf<double> gDk, gDt;           // [n]
  kmx::DevBuf<double> xu;                 // [9n] the rotation CG's (unprojected) iterate
  kmx::DevBuf<double> pmax, mu_in;        // [n_tiles], [nb]
  kmx::DevBuf<int> pcnt;                  // [n_tiles][4]
  kmx::DevBuf<ChRob> rb;                  // [nb]
  kmx::DevBuf<int> rctl;                  // blocks still running
};

struct ChDev {  // what set_graph puts on the device; replaced as a whole
  kmx::DevBuf<int> tile_p0, tile_p1, tile_block, tile_ptr, inc_ptr;
  kmx::DevBuf<uint32_t> inc_other;
  kmx::DevBuf<double> inc_M, inc_t, wk, wt;
  kmx::DevBuf<uint8_t> is_free;
  kmx::DevBuf<double> Dk, Dt, xr, xt, r, d, q, bt, part;
  kmx::DevBuf<ChScal> sc;  // [2][3 nb]: rotations, translations
  kmx::DevBuf<int> ctl;    // [2] (block, row) pairs still running, per stage
  int n_tiles = 0;
  bool have_rob = false;
  ChRobDev rob;
};

}  // namespace

struct kmx_chordal : kmx::StreamCore {
  bool have_graph = false;
  kmx::ChordalGraph g;
  ChDev dev;
  kmx::Event ev[5];
  bool timed = false;
  std::vector<kmx::Event> rev;  // the robust solve's: start, first solve, end, then a pair per GNC pass
  double rstats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool rtimed = false;
};

namespace {

int ch_upload_weights(kmx_chordal* h, ChDev& d, const kmx::ChordalGraph& g, const double* weight) {
  std::vector<double> wk, wt;
  kmx::chordal_record_weights(g, weight, &wk, &wt);
  if (!wk.empty()) {
    KMX_HIP(hipMemcpyAsync(d.wk.get(), wk.data(), wk.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(d.wt.get(), wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(k_ch_diag, dim3((g.n + 255) / 256), dim3(256), 0, h->stream, g.n, d.inc_ptr.get(), d.wk.get(),
                     d.wt.get(), d.Dk.get(), d.Dt.get());
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipStreamSynchronize(h->stream));  // wk / wt are host temporaries
  return KMX_OK;
}

// One stage: the start (residual, who runs), then CG in batches of
// check_every iterations until the device says nobody runs, at most max_it.
template <int W>
int ch_stage(kmx_chordal* h, int stage, double* x, const double* rhs, double rtol, int max_it, int check_every,
             const double* w, const double* D, const ChRob* rb) {
  ChDev& d = h->dev;
  const kmx::ChordalGraph& g = h->g;
  hipStream_t s = h->stream;
  const ChTiles T{d.tile_p0.get(), d.tile_p1.get(), d.tile_block.get()};
  const ChInc I{d.inc_ptr.get(), d.inc_other.get(), w, d.inc_M.get()};
  ChScal* sc = d.sc.get() + (size_t)stage * 3 * g.nb;
  int* ctl = d.ctl.get() + stage;
  const double rtol2 = rtol * rtol;
  const dim3 gt(d.n_tiles), gb(g.nb), wave(CH_TILE);
  KMX_HIP(hipMemsetAsync(ctl, 0, sizeof(int), s));
  hipLaunchKernelGGL((k_ch_apply<W, true>), gt, wave, 0, s, T, I, d.is_free.get(), D, x, rhs, d.r.get(), d.d.get(), sc,
                     ctl, d.part.get(), rb);
  hipLaunchKernelGGL((k_ch_reduce<0>), gb, wave, 0, s, d.tile_ptr.get(), d.part.get(), sc, ctl, rtol2, max_it, rb);
  KMX_HIP(hipGetLastError());
  for (int done = 0; done < max_it;) {
    int running = 0;
    KMX_HIP(hipMemcpyAsync(&running, ctl, sizeof(int), hipMemcpyDeviceToHost, s));
    KMX_HIP(hipStreamSynchronize(s));
    if (running == 0) break;
    const int k = std::min(check_every, max_it - done);
    for (int it = 0; it < k; ++it) {
      hipLaunchKernelGGL((k_ch_apply<W, false>), gt, wave, 0, s, T, I, d.is_free.get(), D, d.d.get(), nullptr,
                         d.q.get(), nullptr, sc, ctl, d.part.get(), nullptr);
      hipLaunchKernelGGL((k_ch_reduce<1>), gb, wave, 0, s, d.tile_ptr.get(), d.part.get(), sc, ctl, rtol2, max_it,
                         nullptr);
      hipLaunchKernelGGL((k_ch_update<W>), gt, wave, 0, s, T, d.is_free.get(), D, x, d.r.get(), d.d.get(), d.q.get(),
                         sc, ctl, d.part.get());
      hipLaunchKernelGGL((k_ch_reduce<2>), gb, wave, 0, s, d.tile_ptr.get(), d.part.get(), sc, ctl, rtol2, max_it,
                         nullptr);
      hipLaunchKernelGGL((k_ch_dir<W>), gt, wave, 0, s, T, d.is_free.get(), D, d.r.get(), d.d.get(), sc, ctl);
    }
    KMX_HIP(hipGetLastError());
    done += k;
  }
  return KMX_OK;
}

}  // namespace

extern "C" int kmx_chordal_create(int device, kmx_chordal** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  std::unique_ptr<kmx_chordal> h(new kmx_chordal());
  int rc;
  if ((rc = h->open(device)) || (rc = kmx::create_events(h->ev))) return rc;
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_destroy(kmx_chordal* h) {
  return kmx::destroy(h);
}

extern "C" int kmx_chordal_set_stream(kmx_chordal* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, true);
}

extern "C" int kmx_chordal_set_graph(kmx_chordal* h, int32_t n_poses, int32_t n_blocks, const int32_t* block_ptr,
                                     int64_t n_edges, const int32_t* src, const int32_t* dst, const double* R,
                                     const double* t, const double* kappa, const double* tau, const double* weight,
                                     int32_t n_anchors, const int32_t* anchors) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  kmx::ChordalGraph g;
  std::string err;
  if (kmx::chordal_build(n_poses, n_blocks, block_ptr, n_edges, src, dst, R, t, kappa, tau, weight, n_anchors,
                         anchors, &g, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_chordal_set_graph: " + err);
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  hipStream_t s = h->stream;
  // built aside, committed by the move below: an error or an exception on its way to KMX_GUARD_END frees only d
  ChDev d;
  d.n_tiles = (int)g.tile_p0.size();
  const size_t n = (size_t)g.n, nrec = g.inc_other.size();
  int rc = KMX_OK;
  if ((rc = d.tile_p0.put(g.tile_p0, s)) || (rc = d.tile_p1.put(g.tile_p1, s)) ||
      (rc = d.tile_block.put(g.tile_block, s)) || (rc = d.tile_ptr.put(g.tile_ptr, s)) ||
      (rc = d.inc_ptr.put(g.inc_ptr, s)) || (rc = d.inc_other.put(g.inc_other, s)) ||
      (rc = d.inc_M.put(g.inc_M, s)) || (rc = d.inc_t.put(g.inc_t, s)) ||
      (rc = d.is_free.put(g.is_free, s)) || (rc = d.wk.alloc(nrec)) || (rc = d.wt.alloc(nrec)) ||
      (rc = d.Dk.alloc(n)) || (rc = d.Dt.alloc(n)) || (rc = d.xr.alloc(9 * n)) || (rc = d.xt.alloc(3 * n)) ||
      (rc = d.r.alloc(9 * n)) || (rc = d.d.alloc(9 * n)) || (rc = d.q.alloc(9 * n)) || (rc = d.bt.alloc(3 * n)) ||
      (rc = d.part.alloc((size_t)CH_NPART * d.n_tiles)) || (rc = d.sc.alloc((size_t)6 * g.nb)) ||
      (rc = d.ctl.alloc(2)) || (rc = ch_upload_weights(h, d, g, weight))) {
    (void)hipStreamSynchronize(s);  // the uploads read g
    return rc;
  }
  // the incidence arrays are only read on the device from here on; the host
  // keeps what set_weights needs
  g.inc_M = std::vector<double>();
  g.inc_t = std::vector<double>();
  h->dev = std::move(d);
  h->g = std::move(g);
  h->have_graph = true;
  h->timed = false;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_set_weights(kmx_chordal* h, const double* weight) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_chordal_set_weights before kmx_chordal_set_graph");
  const kmx::ChordalGraph& g = h->g;
  std::string err;
  if (kmx::chordal_check_weights(g.n, g.m, g.src.data(), g.dst.data(), weight, g.is_free.data(), &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_chordal_set_weights: " + err);
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (int rc = ch_upload_weights(h, h->dev, g, weight)) return rc;
  if (weight)
    h->g.w0.assign(weight, weight + g.m);
  else
    h->g.w0.assign((size_t)g.m, 1.0);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_solve(kmx_chordal* h, const kmx_chordal_params* p, const double* R_init,
                                 const double* t_init, double* R_out, double* t_out, kmx_chordal_block_info* info) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_chordal_solve before kmx_chordal_set_graph");
  KMX_CHECK(R_out && t_out, KMX_EINVAL, "null output");
  double rtol = 1e-10;
  int max_it = 20000, check_every = 50;
  if (p) {
    KMX_CHECK(std::isfinite(p->rtol) && p->rtol >= 0 && p->max_iterations >= 0 && p->check_every >= 0, KMX_EINVAL,
              "kmx_chordal_params: rtol, max_iterations and check_every must be >= 0 (0: the default)");
    if (p->rtol > 0) rtol = p->rtol;
    if (p->max_iterations > 0) max_it = p->max_iterations;
    if (p->check_every > 0) check_every = p->check_every;
  }
  const kmx::ChordalGraph& g = h->g;
  ChDev& d = h->dev;
  const size_t n = (size_t)g.n;
  // the start vectors with the anchors' values in place (R = I, t = 0)
  std::vector<double> xr(9 * n, 0.0), xt(3 * n, 0.0);
  if (R_init) std::memcpy(xr.data(), R_init, 9 * n * sizeof(double));
  if (t_init) std::memcpy(xt.data(), t_init, 3 * n * sizeof(double));
  for (size_t k = 0; k < 9 * n; ++k) KMX_CHECK(std::isfinite(xr[k]), KMX_EINVAL, "R_init not finite");
  for (size_t k = 0; k < 3 * n; ++k) KMX_CHECK(std::isfinite(xt[k]), KMX_EINVAL, "t_init not finite");
  for (size_t q = 0; q < n; ++q)
    if (!g.is_free[q]) {
      for (int k = 0; k < 9; ++k) xr[9 * q + k] = (k % 4 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < 3; ++k) xt[3 * q + k] = 0.0;
    }
  KMX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  KMX_HIP(hipEventRecord(h->ev[0], s));
  KMX_HIP(hipMemcpyAsync(d.xr.get(), xr.data(), 9 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipMemcpyAsync(d.xt.get(), xt.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipEventRecord(h->ev[1], s));
  int rc = ch_stage<3>(h, 0, d.xr.get(), nullptr, rtol, max_it, check_every, d.wk.get(), d.Dk.get(), nullptr);
  if (rc) return rc;
  const dim3 gp((g.n + 255) / 256), bp(256);
  hipLaunchKernelGGL(k_ch_project, gp, bp, 0, s, g.n, d.is_free.get(), d.xr.get());
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipEventRecord(h->ev[2], s));
  hipLaunchKernelGGL(k_ch_rhs_t, gp, bp, 0, s, g.n, d.inc_ptr.get(), d.inc_other.get(), d.wt.get(), d.inc_t.get(),
                     d.is_free.get(), d.xr.get(), d.bt.get());
  KMX_HIP(hipGetLastError());
  rc = ch_stage<1>(h, 1, d.xt.get(), d.bt.get(), rtol, max_it, check_every, d.wt.get(), d.Dt.get(), nullptr);
  if (rc) return rc;
  KMX_HIP(hipEventRecord(h->ev[3], s));
  std::vector<ChScal> sc((size_t)6 * g.nb);
  KMX_HIP(hipMemcpyAsync(R_out, d.xr.get(), 9 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(t_out, d.xt.get(), 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(sc.data(), d.sc.get(), sc.size() * sizeof(ChScal), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipEventRecord(h->ev[4], s));
  KMX_HIP(hipStreamSynchronize(s));
  h->timed = true;
  if (info)
    for (int b = 0; b < g.nb; ++b) {
      kmx_chordal_block_info& o = info[b];
      o.iterations_rot = o.iterations_trans = 0;
      o.converged = 1;
      for (int a = 0; a < 3; ++a) {
        const ChScal& sr = sc[(size_t)3 * b + a];
        const ChScal& st = sc[(size_t)3 * g.nb + 3 * b + a];
        o.iterations_rot = std::max(o.iterations_rot, sr.iters);
        o.iterations_trans = std::max(o.iterations_trans, st.iters);
        o.converged = o.converged && sr.conv && st.conv;
        o.relres_rot[a] = sr.bb > 0 ? std::sqrt(sr.rr / sr.bb) : 0.0;
        o.relres_trans[a] = st.bb > 0 ? std::sqrt(st.rr / st.bb) : 0.0;
      }
    }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_get_timing(kmx_chordal* h, double* ms) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && ms, KMX_EINVAL, "null argument");
  KMX_CHECK(h->timed, KMX_ESTATE, "kmx_chordal_get_timing before kmx_chordal_solve");
  KMX_HIP(hipSetDevice(h->device));
  for (int k = 0; k < 4; ++k) {
    float t = 0.f;
    KMX_HIP(hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]));
    ms[k] = t;
  }
  return KMX_OK;
  KMX_GUARD_END
}

// ---- the robust solve (GNC-TLS around the two stages)
namespace {

// The robust solve's device arrays, at its first call after set_graph.
int ch_robust_reserve(kmx_chordal* h) {
  ChDev& d = h->dev;
  if (d.have_rob) return KMX_OK;
  const kmx::ChordalGraph& g = h->g;
  const size_t n = (size_t)g.n, nrec = g.inc_edge.size();
  std::vector<double> rk(nrec), rt(nrec);
  for (size_t k = 0; k < nrec; ++k) {
    rk[k] = g.kappa[g.inc_edge[k]];
    rt[k] = g.tau[g.inc_edge[k]];
  }
  ChRobDev b;
  int rc = KMX_OK;
  if ((rc = b.rkappa.put(rk, h->stream)) || (rc = b.rtau.put(rt, h->stream)) || (rc = b.rw0.alloc(nrec)) ||
      (rc = b.rfixed.alloc(nrec)) || (rc = b.rg.alloc(nrec)) || (rc = b.gwk.alloc(nrec)) ||
      (rc = b.gwt.alloc(nrec)) || (rc = b.gDk.alloc(n)) || (rc = b.gDt.alloc(n)) || (rc = b.xu.alloc(9 * n)) ||
      (rc = b.pmax.alloc((size_t)d.n_tiles)) || (rc = b.mu_in.alloc((size_t)g.nb)) ||
      (rc = b.pcnt.alloc((size_t)4 * d.n_tiles)) || (rc = b.rb.alloc((size_t)g.nb)) || (rc = b.rctl.alloc(1))) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  KMX_HIP(hipStreamSynchronize(h->stream));  // rk / rt are host temporaries
  d.rob = std::move(b);
  d.have_rob = true;
  return KMX_OK;
}

// w0 and the fixed flag at every record (they can change between two calls).
int ch_robust_upload_edges(kmx_chordal* h, const uint8_t* fixed) {
  ChDev& d = h->dev;
  const kmx::ChordalGraph& g = h->g;
  const size_t nrec = g.inc_edge.size();
  std::vector<double> w0(nrec);
  std::vector<uint8_t> fx;
  for (size_t k = 0; k < nrec; ++k) w0[k] = g.w0[g.inc_edge[k]];
  kmx::chordal_record_fixed(g, fixed, &fx);
  if (nrec) {
    KMX_HIP(hipMemcpyAsync(d.rob.rw0.get(), w0.data(), nrec * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(d.rob.rfixed.get(), fx.data(), nrec, hipMemcpyHostToDevice, h->stream));
  }
  KMX_HIP(hipStreamSynchronize(h->stream));  // host temporaries
  return KMX_OK;
}

ChTiles ch_tiles(const ChDev& d) { return ChTiles{d.tile_p0.get(), d.tile_p1.get(), d.tile_block.get()}; }

ChGnc ch_gnc_args(const ChDev& d) {
  return ChGnc{d.inc_ptr.get(), d.inc_other.get(), d.inc_M.get(), d.inc_t.get(), d.rob.rkappa.get(), d.rob.rtau.get(),
               d.rob.rw0.get(), d.rob.rfixed.get()};
}

// A per-record array back to the caller's edges (an edge's two records hold the same bits).
void ch_records_to_edges(const kmx::ChordalGraph& g, const std::vector<double>& rec, double* out) {
  for (size_t k = 0; k < rec.size(); ++k)
    if (!(g.inc_other[k] & kmx::CH_DIR_OUT)) out[g.inc_edge[k]] = rec[k];
}

int ch_event(kmx_chordal* h, size_t k, hipEvent_t* out) {
  while (h->rev.size() <= k) {
    kmx::Event e;
    if (int rc = e.create()) return rc;
    h->rev.push_back(std::move(e));
  }
  *out = h->rev[k];
  return KMX_OK;
}

}  // namespace

extern "C" int kmx_chordal_residuals(kmx_chordal* h, const double* R, const double* t, const double* mu, double barc,
                                     const uint8_t* fixed, double* r2_out, double* g_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_chordal_residuals before kmx_chordal_set_graph");
  KMX_CHECK(R && t && r2_out, KMX_EINVAL, "null argument");
  KMX_CHECK(!g_out || mu, KMX_EINVAL, "kmx_chordal_residuals: g_out needs mu");
  KMX_CHECK(std::isfinite(barc) && barc >= 0, KMX_EINVAL, "kmx_chordal_residuals: barc must be finite and >= 0");
  const kmx::ChordalGraph& g = h->g;
  const size_t n = (size_t)g.n, nrec = g.inc_edge.size();
  for (size_t k = 0; k < 9 * n; ++k) KMX_CHECK(std::isfinite(R[k]), KMX_EINVAL, "R not finite");
  for (size_t k = 0; k < 3 * n; ++k) KMX_CHECK(std::isfinite(t[k]), KMX_EINVAL, "t not finite");
  if (mu)
    for (int b = 0; b < g.nb; ++b)
      KMX_CHECK(std::isfinite(mu[b]) && mu[b] > 0, KMX_EINVAL, "kmx_chordal_residuals: mu must be finite and > 0");
  const double c = barc > 0 ? barc : 5.0;
  KMX_HIP(hipSetDevice(h->device));
  if (int rc = ch_robust_reserve(h)) return rc;
  if (int rc = ch_robust_upload_edges(h, fixed)) return rc;
  ChDev& d = h->dev;
  hipStream_t s = h->stream;
  // the CG's scratch holds the caller's poses, the robust solve's record
  // weights take r^2 and g: both are rewritten by whoever uses them next
  KMX_HIP(hipMemcpyAsync(d.r.get(), R, 9 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipMemcpyAsync(d.q.get(), t, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  if (mu) KMX_HIP(hipMemcpyAsync(d.rob.mu_in.get(), mu, (size_t)g.nb * sizeof(double), hipMemcpyHostToDevice, s));
  if (d.n_tiles > 0)
    hipLaunchKernelGGL((k_ch_gnc<2>), dim3(d.n_tiles), dim3(CH_TILE), 0, s, ch_tiles(d), ch_gnc_args(d),
                       d.r.get(), d.q.get(), nullptr, mu ? d.rob.mu_in.get() : nullptr, c * c, nullptr, d.rob.gwk.get(),
                       d.rob.gwt.get(), nullptr, nullptr, nullptr, nullptr);
  KMX_HIP(hipGetLastError());
  std::vector<double> rec(nrec);
  if (nrec) KMX_HIP(hipMemcpyAsync(rec.data(), d.rob.gwk.get(), nrec * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipStreamSynchronize(s));
  ch_records_to_edges(g, rec, r2_out);
  if (g_out) {
    if (nrec) KMX_HIP(hipMemcpyAsync(rec.data(), d.rob.gwt.get(), nrec * sizeof(double), hipMemcpyDeviceToHost, s));
    KMX_HIP(hipStreamSynchronize(s));
    ch_records_to_edges(g, rec, g_out);
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_solve_robust(kmx_chordal* h, const kmx_chordal_params* p,
                                        const kmx_chordal_robust_params* rp, const uint8_t* fixed,
                                        const double* R_init, const double* t_init, double* R_out, double* t_out,
                                        double* g_out, kmx_chordal_block_info* info, kmx_chordal_robust_info* rinfo) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_chordal_solve_robust before kmx_chordal_set_graph");
  KMX_CHECK(R_out && t_out, KMX_EINVAL, "null output");
  double rtol = 1e-10;
  int max_it = 20000, check_every = 50;
  if (p) {
    KMX_CHECK(std::isfinite(p->rtol) && p->rtol >= 0 && p->max_iterations >= 0 && p->check_every >= 0, KMX_EINVAL,
              "kmx_chordal_params: rtol, max_iterations and check_every must be >= 0 (0: the default)");
    if (p->rtol > 0) rtol = p->rtol;
    if (p->max_iterations > 0) max_it = p->max_iterations;
    if (p->check_every > 0) check_every = p->check_every;
  }
  kmx::ChordalRobust q;
  std::string err;
  if (kmx::chordal_robust_params(rp, &q, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_chordal_robust_params: " + err);
  const kmx::ChordalGraph& g = h->g;
  if (kmx::chordal_check_fixed(g, fixed, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_chordal_solve_robust: " + err);
  const size_t n = (size_t)g.n, nrec = g.inc_edge.size();
  std::vector<double> xr(9 * n, 0.0), xt(3 * n, 0.0);
  if (R_init) std::memcpy(xr.data(), R_init, 9 * n * sizeof(double));
  if (t_init) std::memcpy(xt.data(), t_init, 3 * n * sizeof(double));
  for (size_t k = 0; k < 9 * n; ++k) KMX_CHECK(std::isfinite(xr[k]), KMX_EINVAL, "R_init not finite");
  for (size_t k = 0; k < 3 * n; ++k) KMX_CHECK(std::isfinite(xt[k]), KMX_EINVAL, "t_init not finite");
  for (size_t a = 0; a < n; ++a)
    if (!g.is_free[a]) {
      for (int k = 0; k < 9; ++k) xr[9 * a + k] = (k % 4 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < 3; ++k) xt[3 * a + k] = 0.0;
    }
  KMX_HIP(hipSetDevice(h->device));
  if (int rc = ch_robust_reserve(h)) return rc;
  if (int rc = ch_robust_upload_edges(h, fixed)) return rc;
  ChDev& d = h->dev;
  hipStream_t s = h->stream;
  const ChTiles T = ch_tiles(d);
  const ChGnc G = ch_gnc_args(d);
  const dim3 gt(d.n_tiles), gb(g.nb), wave(CH_TILE), gp((g.n + 255) / 256), bp(256);
  const double c2 = q.barc * q.barc;
  hipEvent_t e_start, e_first, e_end;
  if (int rc = ch_event(h, 0, &e_start)) return rc;
  if (int rc = ch_event(h, 1, &e_first)) return rc;
  if (int rc = ch_event(h, 2, &e_end)) return rc;
  size_t n_pass = 0;
  h->rtimed = false;
  KMX_HIP(hipEventRecord(e_start, s));
  // the start vectors; the first solve's weights are the handle's, copied: the
  // handle's own wk / wt / D are never written here
  KMX_HIP(hipMemcpyAsync(d.rob.xu.get(), xr.data(), 9 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipMemcpyAsync(d.xr.get(), d.rob.xu.get(), 9 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
  KMX_HIP(hipMemcpyAsync(d.xt.get(), xt.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  if (nrec) {
    KMX_HIP(hipMemcpyAsync(d.rob.gwk.get(), d.wk.get(), nrec * sizeof(double), hipMemcpyDeviceToDevice, s));
    KMX_HIP(hipMemcpyAsync(d.rob.gwt.get(), d.wt.get(), nrec * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  KMX_HIP(hipMemcpyAsync(d.rob.gDk.get(), d.Dk.get(), n * sizeof(double), hipMemcpyDeviceToDevice, s));
  KMX_HIP(hipMemcpyAsync(d.rob.gDt.get(), d.Dt.get(), n * sizeof(double), hipMemcpyDeviceToDevice, s));
  KMX_HIP(hipMemsetAsync(d.rob.rb.get(), 0, (size_t)g.nb * sizeof(ChRob), s));
  KMX_HIP(hipMemsetAsync(d.rob.rctl.get(), 0, sizeof(int), s));
  int solves = 0, running = 0;
  for (int k = 0; k <= q.max_updates; ++k) {
    // 1-4: the rotation stage, the projection, the translations' right-hand side, the translation stage
    int rc = ch_stage<3>(h, 0, d.rob.xu.get(), nullptr, rtol, max_it, check_every, d.rob.gwk.get(), d.rob.gDk.get(),
                         d.rob.rb.get());
    if (rc) return rc;
    if (d.n_tiles > 0)
      hipLaunchKernelGGL(k_ch_project_tiles, gt, wave, 0, s, T, d.rob.rb.get(), d.is_free.get(), d.rob.xu.get(),
                         d.xr.get(), q.start_projected ? 1 : 0);
    hipLaunchKernelGGL(k_ch_rhs_t, gp, bp, 0, s, g.n, d.inc_ptr.get(), d.inc_other.get(), d.rob.gwt.get(),
                       d.inc_t.get(), d.is_free.get(), d.xr.get(), d.bt.get());
    KMX_HIP(hipGetLastError());
    rc = ch_stage<1>(h, 1, d.xt.get(), d.bt.get(), rtol, max_it, check_every, d.rob.gwt.get(), d.rob.gDt.get(),
                     d.rob.rb.get());
    if (rc) return rc;
    ++solves;
    if (k == 0) KMX_HIP(hipEventRecord(e_first, s));
    // 5: the GNC pass and the decision
    hipEvent_t e0, e1;
    if ((rc = ch_event(h, 3 + 2 * n_pass, &e0)) || (rc = ch_event(h, 4 + 2 * n_pass, &e1))) return rc;
    ++n_pass;
    KMX_HIP(hipEventRecord(e0, s));
    if (k == 0) {
      if (d.n_tiles > 0)
        hipLaunchKernelGGL((k_ch_gnc<0>), gt, wave, 0, s, T, G, d.xr.get(), d.xt.get(), d.rob.rb.get(), nullptr, c2,
                           d.rob.rg.get(), nullptr, nullptr, nullptr, nullptr, d.rob.pmax.get(), d.rob.pcnt.get());
      hipLaunchKernelGGL((k_ch_decide<true>), gb, wave, 0, s, d.tile_ptr.get(), d.rob.pmax.get(), d.rob.pcnt.get(),
                         d.rob.rb.get(), d.sc.get(), g.nb, d.rob.rctl.get(), c2, q.mu_init, q.mu_step, 0, 0);
    }
    const int last = k == q.max_updates;
    if (!last && d.n_tiles > 0)
      hipLaunchKernelGGL((k_ch_gnc<1>), gt, wave, 0, s, T, G, d.xr.get(), d.xt.get(), d.rob.rb.get(), nullptr, c2,
                         d.rob.rg.get(), d.rob.gwk.get(), d.rob.gwt.get(), d.rob.gDk.get(), d.rob.gDt.get(),
                         d.rob.pmax.get(), d.rob.pcnt.get());
    hipLaunchKernelGGL((k_ch_decide<false>), gb, wave, 0, s, d.tile_ptr.get(), d.rob.pmax.get(), d.rob.pcnt.get(),
                       d.rob.rb.get(), d.sc.get(), g.nb, d.rob.rctl.get(), c2, q.mu_init, q.mu_step, k > 0, last);
    KMX_HIP(hipGetLastError());
    KMX_HIP(hipEventRecord(e1, s));
    // 6: the one read of the loop
    KMX_HIP(hipMemcpyAsync(&running, d.rob.rctl.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    KMX_HIP(hipStreamSynchronize(s));
    if (running == 0) break;
  }
  std::vector<ChScal> sc((size_t)6 * g.nb);
  std::vector<ChRob> rb((size_t)g.nb);
  std::vector<double> rec(g_out ? nrec : 0);
  KMX_HIP(hipMemcpyAsync(R_out, d.xr.get(), 9 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(t_out, d.xt.get(), 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(sc.data(), d.sc.get(), sc.size() * sizeof(ChScal), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(rb.data(), d.rob.rb.get(), rb.size() * sizeof(ChRob), hipMemcpyDeviceToHost, s));
  if (g_out && nrec) KMX_HIP(hipMemcpyAsync(rec.data(), d.rob.rg.get(), nrec * sizeof(double), hipMemcpyDeviceToHost,
                                            s));
  KMX_HIP(hipEventRecord(e_end, s));
  KMX_HIP(hipStreamSynchronize(s));
  if (g_out) ch_records_to_edges(g, rec, g_out);
  double it_rot = 0, it_trans = 0;
  for (int b = 0; b < g.nb; ++b) {
    it_rot += rb[b].it_rot;
    it_trans += rb[b].it_trans;
    if (rinfo) {
      kmx_chordal_robust_info& o = rinfo[b];
      o.updates = rb[b].updates;
      o.converged = rb[b].conv;
      o.n_kept = rb[b].n1;
      o.n_rejected = rb[b].n0;
      o.n_fractional = rb[b].nf;
      o.reserved = 0;
      o.mu = rb[b].mu;
    }
    if (info) {
      kmx_chordal_block_info& o = info[b];
      o.iterations_rot = o.iterations_trans = 0;
      o.converged = 1;
      for (int a = 0; a < 3; ++a) {
        const ChScal& sr = sc[(size_t)3 * b + a];
        const ChScal& st = sc[(size_t)3 * g.nb + 3 * b + a];
        o.iterations_rot = std::max(o.iterations_rot, sr.iters);
        o.iterations_trans = std::max(o.iterations_trans, st.iters);
        o.converged = o.converged && sr.conv && st.conv;
        o.relres_rot[a] = sr.bb > 0 ? std::sqrt(sr.rr / sr.bb) : 0.0;
        o.relres_trans[a] = st.bb > 0 ? std::sqrt(st.rr / st.bb) : 0.0;
      }
    }
  }
  float ms = 0.f;
  double* st = h->rstats;
  KMX_HIP(hipEventElapsedTime(&ms, e_start, e_end));
  st[0] = ms;
  KMX_HIP(hipEventElapsedTime(&ms, e_start, e_first));
  st[1] = ms;
  st[2] = 0.0;
  for (size_t k = 0; k < n_pass; ++k) {
    KMX_HIP(hipEventElapsedTime(&ms, h->rev[3 + 2 * k], h->rev[4 + 2 * k]));
    st[2] += ms;
  }
  st[3] = (double)n_pass;
  st[4] = it_rot;
  st[5] = it_trans;
  st[6] = solves;
  st[7] = 0.0;
  h->rtimed = true;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_get_robust_stats(kmx_chordal* h, double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->rtimed, KMX_ESTATE, "kmx_chordal_get_robust_stats before kmx_chordal_solve_robust");
  for (int k = 0; k < 8; ++k) out[k] = h->rstats[k];
  return KMX_OK;
  KMX_GUARD_END
}
