// dgraph.hip — kmx_dgraph_*: the deformation graph's optimisation on the
// device (include/kmx_abi.h "Deformation graph optimisation"):
// Levenberg-Marquardt over (R_i, t_i) of every free node, each step solved by
// conjugate gradients preconditioned with the inverse 6x6 diagonal blocks.
// All arithmetic is fp64 and this file is compiled with -ffp-contract=off.
//
// Layout. Per node: rest pose, pose, trial pose, prior, b [6], the diagonal
// block's upper triangle [21], its damped inverse [21] and the CG vectors
// x, r, z, p, q [6]. Per incidence record (CSR by node, records in edge order,
// graph_host.h): `other` with the tail bit (4 B), w (8 B) and a_e = R_i d_e of
// the edge's source i (24 B): the 36 B the matrix-free product reads; d_e
// (24 B) is read only when a_e is re-formed.
//
// Sums are ordered. A node (a lane) adds its records in CSR order; a tile (64
// consecutive nodes, one wave) reduces with a fixed shuffle tree; one wave
// sums the tile partials, lane l taking tiles l, l + 64, ..., then the same
// tree (k_dg_reduce). No floating-point atomics. No grid barrier, no
// persistent kernel, no device-side wait: the host enqueues check_every CG
// iterations at a time and reads one word in between; every CG launch tests
// that word first and returns at once when the solve has stopped, and the
// solve stops itself at cg_max_iterations, so nothing depends on check_every.
// The LM decision is taken on the device (k_dg_decide) into the state record
// that the host reads once per outer iteration.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "common.h"
#include "dgraph_host.h"

namespace {
using kmx::DG_TILE;

struct DgState {
  double f, f_trial, lambda, lambda_used, bb;  // bb: |b|^2 at the current point
  double cg_bb, rr, rz, alpha, beta;
  int cg_active, cg_iters;
  int accepted, stop, iter, n_accepted;
};

using kmx::wave_sum;  // lane 0 holds the sum; fixed tree

__host__ __device__ constexpr int tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }  // i <= j

// z = S r for the symmetric 6x6 S given by its upper triangle
__device__ __forceinline__ void dg_symv(const double (&S)[21], const double (&r)[6], double (&z)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s += S[i <= j ? tri(i, j) : tri(j, i)] * r[j];
    z[i] = s;
  }
}

// d_e = Rrest_i^T (g_j - g_i) of every record, i the edge's source
__global__ void k_dg_edges(int n, const int* __restrict__ ptr, const uint32_t* __restrict__ other,
                           const double* __restrict__ Rrest, const double* __restrict__ g, double* __restrict__ d) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  for (int k = ptr[p]; k < ptr[p + 1]; ++k) {
    const uint32_t rec = other[k];
    const int o = (int)(rec & 0x7fffffffu);
    const bool tail = (rec & kmx::GRAPH_TAIL) != 0;
    const int i = tail ? p : o, j = tail ? o : p;
    const double* R = Rrest + (size_t)9 * i;
    double dg[3];
    for (int c = 0; c < 3; ++c) dg[c] = g[(size_t)3 * j + c] - g[(size_t)3 * i + c];
    for (int c = 0; c < 3; ++c) {
      double v = R[c] * dg[0];
      v += R[3 + c] * dg[1];
      v += R[6 + c] * dg[2];
      d[(size_t)3 * k + c] = v;
    }
  }
}

// hard nodes sit at their priors
__global__ void k_dg_pin(int n, const uint8_t* __restrict__ mode, const double* __restrict__ Rhat,
                         const double* __restrict__ that, double* __restrict__ R, double* __restrict__ t) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || mode[p] != 2) return;
  for (int c = 0; c < 9; ++c) R[(size_t)9 * p + c] = Rhat[(size_t)9 * p + c];
  for (int c = 0; c < 3; ++c) t[(size_t)3 * p + c] = that[(size_t)3 * p + c];
}

// rows of hard nodes <- 0
__global__ void k_dg_mask(int n, const uint8_t* __restrict__ mode, double* __restrict__ v) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || mode[p] != 2) return;
  for (int c = 0; c < 6; ++c) v[(size_t)6 * p + c] = 0.0;
}

struct DgRec {
  const int* ptr;
  const uint32_t* other;
  const double* w;
  const double* d;
  double* a;
};

struct DgPrior {
  const uint8_t* mode;
  const double *Rhat, *that, *kappa, *tau;
};

// A lane owns a node of the tile and walks its records at the poses (R, t).
//   FULL: re-forms every record's a_e, and writes the node's gradient b, the
//         upper triangle of its diagonal block of J^T J and the tile's
//         partials of the cost and of |b|^2 (k_dg_linearize).
//   else: the tile's cost partial only (k_dg_cost: the trial point). The cost
//         is the same code in both, so an accepted trial cost is the next
//         iteration's cost bit for bit.
// An edge's cost is counted at its source's record.
template <bool FULL>
__global__ __launch_bounds__(DG_TILE) void k_dg_linearize(int n, DgRec I, DgPrior P, const double* __restrict__ R,
                                                          const double* __restrict__ t, double* __restrict__ b,
                                                          double* __restrict__ blk, double* __restrict__ part) {
  const int tile = blockIdx.x;
  const int p = tile * DG_TILE + (int)threadIdx.x;
  double cost = 0.0, bsq = 0.0;
  if (p < n) {
    double Rp[9], tp[3];
    for (int c = 0; c < 9; ++c) Rp[c] = R[(size_t)9 * p + c];
    for (int c = 0; c < 3; ++c) tp[c] = t[(size_t)3 * p + c];
    double bw[3] = {0.0, 0.0, 0.0}, bd[3] = {0.0, 0.0, 0.0};
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // 00 01 02 11 12 22
    double s[3] = {0.0, 0.0, 0.0}, cc = 0.0;
    const int k1 = I.ptr[p + 1];
    for (int k = I.ptr[p]; k < k1; ++k) {
      const double w = I.w[k];
      if (w == 0.0) continue;
      const uint32_t rec = I.other[k];
      const int o = (int)(rec & 0x7fffffffu);
      const bool tail = (rec & kmx::GRAPH_TAIL) != 0;
      double Ri[9];
      if (tail) {
#pragma unroll
        for (int c = 0; c < 9; ++c) Ri[c] = Rp[c];
      } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) Ri[c] = R[(size_t)9 * o + c];
      }
      const double d0 = I.d[(size_t)3 * k], d1 = I.d[(size_t)3 * k + 1], d2 = I.d[(size_t)3 * k + 2];
      double a[3], r[3];
      for (int c = 0; c < 3; ++c) a[c] = Ri[3 * c] * d0 + Ri[3 * c + 1] * d1 + Ri[3 * c + 2] * d2;
      if (FULL)
        for (int c = 0; c < 3; ++c) I.a[(size_t)3 * k + c] = a[c];
      if (tail) {
        for (int c = 0; c < 3; ++c) r[c] = (a[c] + tp[c]) - t[(size_t)3 * o + c];
        cost += w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (FULL) {
          bw[0] += w * (a[1] * r[2] - a[2] * r[1]);
          bw[1] += w * (a[2] * r[0] - a[0] * r[2]);
          bw[2] += w * (a[0] * r[1] - a[1] * r[0]);
          for (int c = 0; c < 3; ++c) bd[c] += w * r[c];
          A[0] += w * (a[1] * a[1] + a[2] * a[2]);
          A[1] -= w * (a[0] * a[1]);
          A[2] -= w * (a[0] * a[2]);
          A[3] += w * (a[0] * a[0] + a[2] * a[2]);
          A[4] -= w * (a[1] * a[2]);
          A[5] += w * (a[0] * a[0] + a[1] * a[1]);
          for (int c = 0; c < 3; ++c) s[c] += w * a[c];
          cc += w;
        }
      } else if (FULL) {
        for (int c = 0; c < 3; ++c) r[c] = (a[c] + t[(size_t)3 * o + c]) - tp[c];
        for (int c = 0; c < 3; ++c) bd[c] -= w * r[c];
        cc += w;
      }
    }
    const int mode = P.mode[p];
    if (mode == 1) {
      const double kap = P.kappa[p], tau = P.tau[p];
      double E[9], et[3], se = 0.0, st = 0.0;
      for (int c = 0; c < 9; ++c) {
        E[c] = Rp[c] - P.Rhat[(size_t)9 * p + c];
        se += E[c] * E[c];
      }
      for (int c = 0; c < 3; ++c) {
        et[c] = tp[c] - P.that[(size_t)3 * p + c];
        st += et[c] * et[c];
      }
      cost += kap * se + tau * st;
      if (FULL) {
        // kappa sum over the columns c of R_c x E_c
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        for (int c = 0; c < 3; ++c) {
          x0 += Rp[3 + c] * E[6 + c] - Rp[6 + c] * E[3 + c];
          x1 += Rp[6 + c] * E[c] - Rp[c] * E[6 + c];
          x2 += Rp[c] * E[3 + c] - Rp[3 + c] * E[c];
        }
        bw[0] += kap * x0;
        bw[1] += kap * x1;
        bw[2] += kap * x2;
        for (int c = 0; c < 3; ++c) bd[c] += tau * et[c];
        A[0] += 2.0 * kap;
        A[3] += 2.0 * kap;
        A[5] += 2.0 * kap;
        cc += tau;
      }
    }
    if (FULL) {
      const bool hard = mode == 2;
      double o[21] = {A[0], A[1], A[2], 0.0, -s[2], s[1], A[3], A[4], s[2], 0.0, -s[0],
                      A[5], -s[1], s[0], 0.0, cc, 0.0, 0.0, cc, 0.0, cc};
      for (int c = 0; c < 21; ++c) blk[(size_t)21 * p + c] = hard ? 0.0 : o[c];
      for (int c = 0; c < 3; ++c) {
        const double u = hard ? 0.0 : bw[c], v = hard ? 0.0 : bd[c];
        b[(size_t)6 * p + c] = u;
        b[(size_t)6 * p + 3 + c] = v;
        bsq += u * u;
        bsq += v * v;
      }
    }
  }
  cost = wave_sum(cost);
  if (FULL) bsq = wave_sum(bsq);
  if (threadIdx.x == 0) {
    part[(size_t)2 * tile] = cost;
    if (FULL) part[(size_t)2 * tile + 1] = bsq;
  }
}

// Minv = (block + lambda I)^-1 by Cholesky, every loop unrolled so that no
// array is indexed dynamically; 0 at hard nodes.
__global__ __launch_bounds__(256) void k_dg_precond(int n, const uint8_t* __restrict__ mode,
                                                    const double* __restrict__ blk, const DgState* __restrict__ st,
                                                    double* __restrict__ Minv) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  double out[21];
  if (mode[p] == 2) {
#pragma unroll
    for (int c = 0; c < 21; ++c) out[c] = 0.0;
  } else {
    const double lam = st->lambda;
    double U[21], L[6][6], Li[6][6];
#pragma unroll
    for (int c = 0; c < 21; ++c) U[c] = blk[(size_t)21 * p + c];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = U[tri(j, j)] + lam;
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
      L[j][j] = sqrt(s);
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double v = U[tri(j, i)];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
        L[i][j] = v / L[j][j];
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      Li[j][j] = 1.0 / L[j][j];
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double v = 0.0;
#pragma unroll
        for (int k = j; k < i; ++k) v -= L[i][k] * Li[k][j];
        Li[i][j] = v / L[i][i];
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = j; k < 6; ++k) v += Li[k][i] * Li[k][j];
        out[tri(i, j)] = v;
      }
  }
#pragma unroll
  for (int c = 0; c < 21; ++c) Minv[(size_t)21 * p + c] = out[c];
}

// x = 0, r = -b, z = Minv r, p = z; the tile's partials <r,r>, <r,z>
__global__ __launch_bounds__(DG_TILE) void k_dg_cg_init(int n, const double* __restrict__ b,
                                                        const double* __restrict__ Minv, double* __restrict__ x,
                                                        double* __restrict__ r, double* __restrict__ z,
                                                        double* __restrict__ pv, double* __restrict__ part) {
  const int tile = blockIdx.x;
  const int p = tile * DG_TILE + (int)threadIdx.x;
  double srr = 0.0, srz = 0.0;
  if (p < n) {
    double S[21], rv[6], zv[6];
#pragma unroll
    for (int c = 0; c < 21; ++c) S[c] = Minv[(size_t)21 * p + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) rv[c] = -b[(size_t)6 * p + c];
    dg_symv(S, rv, zv);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      x[(size_t)6 * p + c] = 0.0;
      r[(size_t)6 * p + c] = rv[c];
      z[(size_t)6 * p + c] = zv[c];
      pv[(size_t)6 * p + c] = zv[c];
      srr += rv[c] * rv[c];
      srz += rv[c] * zv[c];
    }
  }
  srr = wave_sum(srr);
  srz = wave_sum(srz);
  if (threadIdx.x == 0) {
    part[(size_t)2 * tile] = srr;
    part[(size_t)2 * tile + 1] = srz;
  }
}

// q = (J^T J + lambda I) v, matrix-free from the records, and the tile's
// partial <v, q>. Rows of hard nodes are 0 in v and stay 0 in q.
//   EVAL: kmx_dgraph_eval's J^T J v: lambda = 0, no stop word, no partial.
template <bool EVAL>
__global__ __launch_bounds__(DG_TILE) void k_dg_apply(int n, DgRec I, DgPrior P, const double* __restrict__ v,
                                                      double* __restrict__ q, const DgState* __restrict__ st,
                                                      double* __restrict__ part) {
  if (!EVAL && !st->cg_active) return;
  const int tile = blockIdx.x;
  const int p = tile * DG_TILE + (int)threadIdx.x;
  double spq = 0.0;
  if (p < n) {
    const int mode = P.mode[p];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mode != 2) {
      const double lam = EVAL ? 0.0 : st->lambda;
      double vp[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) vp[c] = v[(size_t)6 * p + c];
      const int k1 = I.ptr[p + 1];
      for (int k = I.ptr[p]; k < k1; ++k) {
        const double w = I.w[k];
        if (w == 0.0) continue;
        const uint32_t rec = I.other[k];
        const int o = (int)(rec & 0x7fffffffu);
        const double a0 = I.a[(size_t)3 * k], a1 = I.a[(size_t)3 * k + 1], a2 = I.a[(size_t)3 * k + 2];
        const double* vo = v + (size_t)6 * o;
        if (rec & kmx::GRAPH_TAIL) {  // u = omega_p x a + delta_p - delta_o
          const double u0 = ((vp[1] * a2 - vp[2] * a1) + vp[3]) - vo[3];
          const double u1 = ((vp[2] * a0 - vp[0] * a2) + vp[4]) - vo[4];
          const double u2 = ((vp[0] * a1 - vp[1] * a0) + vp[5]) - vo[5];
          acc[0] += w * (a1 * u2 - a2 * u1);
          acc[1] += w * (a2 * u0 - a0 * u2);
          acc[2] += w * (a0 * u1 - a1 * u0);
          acc[3] += w * u0;
          acc[4] += w * u1;
          acc[5] += w * u2;
        } else {  // u = omega_o x a + delta_o - delta_p
          const double u0 = ((vo[1] * a2 - vo[2] * a1) + vo[3]) - vp[3];
          const double u1 = ((vo[2] * a0 - vo[0] * a2) + vo[4]) - vp[4];
          const double u2 = ((vo[0] * a1 - vo[1] * a0) + vo[5]) - vp[5];
          acc[3] -= w * u0;
          acc[4] -= w * u1;
          acc[5] -= w * u2;
        }
      }
      if (mode == 1) {
        const double k2 = 2.0 * P.kappa[p], tau = P.tau[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc[c] += k2 * vp[c];
          acc[3 + c] += tau * vp[3 + c];
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        acc[c] += lam * vp[c];
        spq += vp[c] * acc[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) q[(size_t)6 * p + c] = acc[c];
  }
  if (!EVAL) {
    spq = wave_sum(spq);
    if (threadIdx.x == 0) part[(size_t)2 * tile] = spq;
  }
}

// x += alpha p, r -= alpha q, z = Minv r; the tile's partials <r,r>, <r,z>
__global__ __launch_bounds__(DG_TILE) void k_dg_update(int n, const double* __restrict__ Minv, double* __restrict__ x,
                                                       double* __restrict__ r, double* __restrict__ z,
                                                       const double* __restrict__ pv, const double* __restrict__ q,
                                                       const DgState* __restrict__ st, double* __restrict__ part) {
  if (!st->cg_active) return;
  const double alpha = st->alpha;
  const int tile = blockIdx.x;
  const int p = tile * DG_TILE + (int)threadIdx.x;
  double srr = 0.0, srz = 0.0;
  if (p < n) {
    double S[21], rv[6], zv[6];
#pragma unroll
    for (int c = 0; c < 21; ++c) S[c] = Minv[(size_t)21 * p + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      x[(size_t)6 * p + c] += alpha * pv[(size_t)6 * p + c];
      rv[c] = r[(size_t)6 * p + c] - alpha * q[(size_t)6 * p + c];
      r[(size_t)6 * p + c] = rv[c];
    }
    dg_symv(S, rv, zv);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      z[(size_t)6 * p + c] = zv[c];
      srr += rv[c] * rv[c];
      srz += rv[c] * zv[c];
    }
  }
  srr = wave_sum(srr);
  srz = wave_sum(srz);
  if (threadIdx.x == 0) {
    part[(size_t)2 * tile] = srr;
    part[(size_t)2 * tile + 1] = srz;
  }
}

// p = z + beta p
__global__ __launch_bounds__(256) void k_dg_dir(int n6, const double* __restrict__ z, double* __restrict__ pv,
                                                const DgState* __restrict__ st) {
  if (!st->cg_active) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n6) return;
  pv[k] = z[k] + st->beta * pv[k];
}

// The tile partials, summed by one wave in a fixed order, and what follows
// from the sums.
//   PHASE 0: <r,r>, <r,z> of the CG's start: whether it runs at all
//   PHASE 1: <p,q>: alpha
//   PHASE 2: <r,r>, <r,z> after the update: beta, the stop test, the count
//   PHASE 3: the cost and |b|^2 of a linearisation (flag: the cost is stored)
//   PHASE 4: the trial cost
template <int PHASE>
__global__ __launch_bounds__(64) void k_dg_reduce(const double* __restrict__ part, int n_tiles, DgState* __restrict__ st,
                                                  double rtol2, int max_it, int flag) {
  if ((PHASE == 1 || PHASE == 2) && !st->cg_active) return;
  const int lane = threadIdx.x;
  constexpr int NQ = (PHASE == 1 || PHASE == 4) ? 1 : 2;
  double v[NQ];
  for (int qd = 0; qd < NQ; ++qd) {
    double u = 0.0;
    for (int t = lane; t < n_tiles; t += 64) u += part[(size_t)2 * t + qd];
    v[qd] = wave_sum(u);
  }
  if (lane != 0) return;
  if constexpr (PHASE == 0) {
    st->cg_bb = v[0];
    st->rr = v[0];
    st->rz = v[1];
    st->alpha = st->beta = 0.0;
    st->cg_iters = 0;
    st->cg_active = (v[0] > 0.0 && !(v[0] <= rtol2 * v[0]) && max_it > 0) ? 1 : 0;
  } else if constexpr (PHASE == 1) {
    if (v[0] > 0.0)
      st->alpha = st->rz / v[0];
    else  // the matrix is positive definite: p = 0 or a NaN; stop here
      st->cg_active = 0;
  } else if constexpr (PHASE == 2) {
    st->cg_iters += 1;
    st->beta = v[1] / st->rz;
    st->rz = v[1];
    st->rr = v[0];
    if (v[0] <= rtol2 * st->cg_bb || st->cg_iters >= max_it) st->cg_active = 0;
  } else if constexpr (PHASE == 3) {
    if (flag) st->f = v[0];
    st->bb = v[1];
  } else {
    st->f_trial = v[0];
  }
}

// The trial point: R+ = Exp(omega) R (Rodrigues), t+ = t + delta. A node whose
// step is exactly 0 (every hard node) is copied.
__global__ __launch_bounds__(256) void k_dg_retract(int n, const double* __restrict__ x, const double* __restrict__ R,
                                                    const double* __restrict__ t, double* __restrict__ Rt,
                                                    double* __restrict__ tt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double w0 = x[(size_t)6 * p], w1 = x[(size_t)6 * p + 1], w2 = x[(size_t)6 * p + 2];
  for (int c = 0; c < 3; ++c) tt[(size_t)3 * p + c] = t[(size_t)3 * p + c] + x[(size_t)6 * p + 3 + c];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  if (th2 == 0.0) {
    for (int c = 0; c < 9; ++c) Rt[(size_t)9 * p + c] = R[(size_t)9 * p + c];
    return;
  }
  double A, B;
  if (th2 < 1e-8) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    const double th = sqrt(th2);
    A = sin(th) / th;
    B = (1.0 - cos(th)) / th2;
  }
  // E = I + A [w]x + B [w]x^2, [w]x^2 = w w^T - |w|^2 I
  const double E[9] = {1.0 + B * (w0 * w0 - th2), B * (w0 * w1) - A * w2,    B * (w0 * w2) + A * w1,
                       B * (w0 * w1) + A * w2,    1.0 + B * (w1 * w1 - th2), B * (w1 * w2) - A * w0,
                       B * (w0 * w2) - A * w1,    B * (w1 * w2) + A * w0,    1.0 + B * (w2 * w2 - th2)};
  double Rp[9];
  for (int c = 0; c < 9; ++c) Rp[c] = R[(size_t)9 * p + c];
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c)
      Rt[(size_t)9 * p + 3 * a + c] = E[3 * a] * Rp[c] + E[3 * a + 1] * Rp[3 + c] + E[3 * a + 2] * Rp[6 + c];
}

// The Levenberg-Marquardt decision, one lane.
__global__ void k_dg_decide(DgState* __restrict__ st, double factor, double lmin, double lmax, double rel_tol,
                            double abs_tol, int max_it) {
  const double f = st->f, fp = st->f_trial, lam = st->lambda;
  st->lambda_used = lam;
  st->iter += 1;
  const bool acc = fp < f;  // false for a NaN
  int stop = 0;
  if (acc) {
    st->n_accepted += 1;
    const double l = lam / factor;
    st->lambda = l > lmin ? l : lmin;
    if (fp <= abs_tol)
      stop = 2;
    else if (f - fp <= rel_tol * f)
      stop = 1;
    st->f = fp;
  } else {
    st->lambda = lam * factor;
    if (st->lambda > lmax) stop = 4;
  }
  if (!stop && st->iter >= max_it) stop = 3;
  st->accepted = acc ? 1 : 0;
  st->stop = stop;
}

struct DgDev {  // what set_graph puts on the device; replaced as a whole
  kmx::DevBuf<int> ptr;
  kmx::DevBuf<uint32_t> other;
  kmx::DevBuf<double> rec_w, rec_d, rec_a;
  kmx::DevBuf<double> Rrest, g, R, t, Rt, tt;
  kmx::DevBuf<uint8_t> mode;
  kmx::DevBuf<double> Rhat, that, kappa, tau;
  kmx::DevBuf<double> b, blk, Minv, x, r, z, p, q, part;
  kmx::DevBuf<DgState> st;
};

}  // namespace

struct kmx_dgraph : kmx::StreamCore {
  bool have_graph = false, have_priors = false;
  kmx::DgGraph G;
  kmx::DgPriors P;
  DgDev dev;
  kmx::Event ev[6];
  double ms[5] = {0, 0, 0, 0, 0};  // [4]: the product kernel of the last J^T J evaluation
  std::vector<kmx_dgraph_log_entry> log;
};

namespace {

inline dim3 dg_grid(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// hard nodes to their priors, a_e, b, the blocks, the cost and |b|^2 at the current poses
int dg_linearize(kmx_dgraph* h, int store_cost) {
  DgDev& d = h->dev;
  const int n = h->G.n;
  const DgRec I{d.ptr.get(), d.other.get(), d.rec_w.get(), d.rec_d.get(), d.rec_a.get()};
  const DgPrior P{d.mode.get(), d.Rhat.get(), d.that.get(), d.kappa.get(), d.tau.get()};
  hipLaunchKernelGGL((k_dg_linearize<true>), dim3(h->G.n_tiles), dim3(DG_TILE), 0, h->stream, n, I, P, d.R.get(),
                     d.t.get(), d.b.get(), d.blk.get(), d.part.get());
  hipLaunchKernelGGL((k_dg_reduce<3>), dim3(1), dim3(64), 0, h->stream, d.part.get(), h->G.n_tiles, d.st.get(), 0.0, 0,
                     store_cost);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

int dg_pin(kmx_dgraph* h) {
  DgDev& d = h->dev;
  hipLaunchKernelGGL(k_dg_pin, dg_grid(h->G.n, 256), dim3(256), 0, h->stream, h->G.n, d.mode.get(), d.Rhat.get(),
                     d.that.get(), d.R.get(), d.t.get());
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

int dg_read_state(kmx_dgraph* h, DgState* s) {
  KMX_HIP(hipMemcpyAsync(s, h->dev.st.get(), sizeof(DgState), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

}  // namespace

extern "C" int kmx_dgraph_create(int device, kmx_dgraph** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  std::unique_ptr<kmx_dgraph> h(new kmx_dgraph());
  int rc;
  if ((rc = h->open(device)) || (rc = kmx::create_events(h->ev))) return rc;
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_destroy(kmx_dgraph* h) {
  return kmx::destroy(h);
}

extern "C" int kmx_dgraph_set_stream(kmx_dgraph* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, true);
}

extern "C" int kmx_dgraph_set_graph(kmx_dgraph* h, int32_t n, const double* Rrest, const double* g, int64_t m,
                                    const int32_t* src, const int32_t* dst, const double* w) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  kmx::DgGraph G;
  std::string err;
  if (int rc = kmx::dg_build(n, Rrest, g, m, src, dst, w, &G, &err)) return kmx::fail(rc,
                                                                                      "kmx_dgraph_set_graph: " + err);
  std::vector<double> rec_w;
  kmx::dg_record_weights(G, G.w.data(), &rec_w);
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  hipStream_t s = h->stream;
  // built aside, committed by the move below: an error or an exception on its way to KMX_GUARD_END frees only d
  DgDev d;
  const size_t nn = (size_t)n, nrec = G.inc_other.size(), nt = (size_t)G.n_tiles;
  int rc = KMX_OK;
  if ((rc = d.ptr.put(G.inc_ptr, s)) || (rc = d.other.put(G.inc_other, s)) ||
      (rc = d.rec_w.put(rec_w, s)) || (rc = d.rec_d.alloc(3 * nrec)) || (rc = d.rec_a.alloc(3 * nrec)) ||
      (rc = d.Rrest.put(Rrest, 9 * nn, s)) || (rc = d.g.put(g, 3 * nn, s)) || (rc = d.R.put(Rrest, 9 * nn, s)) ||
      (rc = d.t.put(g, 3 * nn, s)) || (rc = d.Rt.alloc(9 * nn)) || (rc = d.tt.alloc(3 * nn)) ||
      (rc = d.mode.alloc(nn)) || (rc = d.Rhat.alloc(9 * nn)) || (rc = d.that.alloc(3 * nn)) ||
      (rc = d.kappa.alloc(nn)) || (rc = d.tau.alloc(nn)) || (rc = d.b.alloc(6 * nn)) || (rc = d.blk.alloc(21 * nn)) ||
      (rc = d.Minv.alloc(21 * nn)) || (rc = d.x.alloc(6 * nn)) || (rc = d.r.alloc(6 * nn)) ||
      (rc = d.z.alloc(6 * nn)) || (rc = d.p.alloc(6 * nn)) || (rc = d.q.alloc(6 * nn)) ||
      (rc = d.part.alloc(2 * nt)) || (rc = d.st.alloc(1))) {
    (void)hipStreamSynchronize(s);  // the uploads read the caller's arrays
    return rc;
  }
  hipError_t e = hipSuccess;
  if (n > 0) {
    hipLaunchKernelGGL(k_dg_edges, dg_grid(n, 256), dim3(256), 0, s, n, d.ptr.get(), d.other.get(), d.Rrest.get(),
                       d.g.get(), d.rec_d.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemsetAsync(d.mode.get(), 0, std::max<size_t>(nn, 1), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the caller's arrays and rec_w are free again
  if (e != hipSuccess) return kmx::fail(KMX_EHIP, std::string("kmx_dgraph_set_graph: ") + hipGetErrorString(e));
  h->dev = std::move(d);
  h->G = std::move(G);
  h->P = kmx::DgPriors();
  h->have_graph = true;
  h->have_priors = false;
  h->log.clear();
  for (double& v : h->ms) v = 0.0;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_set_weights(kmx_dgraph* h, const double* w) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_dgraph_set_weights before kmx_dgraph_set_graph");
  const kmx::DgGraph& G = h->G;
  std::string err;
  if (int rc = kmx::dg_check_weights(G.m, w, &err)) return kmx::fail(rc, "kmx_dgraph_set_weights: " + err);
  if (h->have_priors)
    if (int rc = kmx::dg_check_posed(G.n, G.m, G.src.data(), G.dst.data(), w, h->P, &err))
      return kmx::fail(rc, "kmx_dgraph_set_weights: " + err);
  std::vector<double> rec_w;
  kmx::dg_record_weights(G, w, &rec_w);
  KMX_HIP(hipSetDevice(h->device));
  if (!rec_w.empty())
    KMX_HIP(hipMemcpyAsync(h->dev.rec_w.get(), rec_w.data(), rec_w.size() * sizeof(double), hipMemcpyHostToDevice,
                           h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (w)
    h->G.w.assign(w, w + G.m);
  else
    h->G.w.assign((size_t)G.m, 1.0);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_set_priors(kmx_dgraph* h, const uint8_t* mode, const double* Rhat, const double* that,
                                     const double* kappa, const double* tau) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_dgraph_set_priors before kmx_dgraph_set_graph");
  const kmx::DgGraph& G = h->G;
  kmx::DgPriors P;
  std::string err;
  if (int rc = kmx::dg_check_priors(G.n, mode, Rhat, that, kappa, tau, &P, &err))
    return kmx::fail(rc, "kmx_dgraph_set_priors: " + err);
  if (int rc = kmx::dg_check_posed(G.n, G.m, G.src.data(), G.dst.data(), G.w.data(), P, &err))
    return kmx::fail(rc, "kmx_dgraph_set_priors: " + err);
  KMX_HIP(hipSetDevice(h->device));
  const size_t nn = (size_t)G.n;
  hipStream_t s = h->stream;
  DgDev& d = h->dev;
  if (nn) {
    KMX_HIP(hipMemcpyAsync(d.mode.get(), P.mode.data(), nn, hipMemcpyHostToDevice, s));
    KMX_HIP(hipMemcpyAsync(d.Rhat.get(), P.Rhat.data(), 9 * nn * sizeof(double), hipMemcpyHostToDevice, s));
    KMX_HIP(hipMemcpyAsync(d.that.get(), P.that.data(), 3 * nn * sizeof(double), hipMemcpyHostToDevice, s));
    KMX_HIP(hipMemcpyAsync(d.kappa.get(), P.kappa.data(), nn * sizeof(double), hipMemcpyHostToDevice, s));
    KMX_HIP(hipMemcpyAsync(d.tau.get(), P.tau.data(), nn * sizeof(double), hipMemcpyHostToDevice, s));
  }
  KMX_HIP(hipStreamSynchronize(s));
  h->P = std::move(P);
  h->have_priors = true;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_set_poses(kmx_dgraph* h, const double* R, const double* t) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_dgraph_set_poses before kmx_dgraph_set_graph");
  KMX_CHECK((R == nullptr) == (t == nullptr), KMX_EINVAL, "R and t: both or neither");
  const size_t nn = (size_t)h->G.n;
  if (R)
    KMX_CHECK(kmx::dg_all_finite(R, 9 * nn) && kmx::dg_all_finite(t, 3 * nn), KMX_EINVAL, "pose is not finite");
  KMX_HIP(hipSetDevice(h->device));
  if (nn) {
    const hipMemcpyKind kind = R ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    KMX_HIP(hipMemcpyAsync(h->dev.R.get(), R ? R : h->dev.Rrest.get(), 9 * nn * sizeof(double), kind, h->stream));
    KMX_HIP(hipMemcpyAsync(h->dev.t.get(), t ? t : h->dev.g.get(), 3 * nn * sizeof(double), kind, h->stream));
  }
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_get_poses(kmx_dgraph* h, double* R, double* t) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_dgraph_get_poses before kmx_dgraph_set_graph");
  const size_t nn = (size_t)h->G.n;
  KMX_CHECK(nn == 0 || (R && t), KMX_EINVAL, "null output");
  KMX_HIP(hipSetDevice(h->device));
  if (nn) {
    KMX_HIP(hipMemcpyAsync(R, h->dev.R.get(), 9 * nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KMX_HIP(hipMemcpyAsync(t, h->dev.t.get(), 3 * nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_eval(kmx_dgraph* h, int32_t what, const double* v, double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(what >= KMX_DGRAPH_EVAL_COST && what <= KMX_DGRAPH_EVAL_BLOCKS, KMX_EUNSUP, "unknown evaluation");
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(out, KMX_EINVAL, "null output");
  KMX_CHECK(what != KMX_DGRAPH_EVAL_JTJ || v || !h->have_graph || h->G.n == 0, KMX_EINVAL, "null v");
  KMX_CHECK(h->have_graph && h->have_priors, KMX_ESTATE, "kmx_dgraph_eval before set_graph and set_priors");
  const int n = h->G.n;
  const size_t nn = (size_t)n;
  if (what == KMX_DGRAPH_EVAL_JTJ) KMX_CHECK(kmx::dg_all_finite(v, 6 * nn), KMX_EINVAL, "v is not finite");
  if (n == 0) {
    if (what == KMX_DGRAPH_EVAL_COST) *out = 0.0;
    return KMX_OK;
  }
  KMX_HIP(hipSetDevice(h->device));
  DgDev& d = h->dev;
  hipStream_t s = h->stream;
  if (int rc = dg_pin(h)) return rc;
  if (int rc = dg_linearize(h, 1)) return rc;
  if (what == KMX_DGRAPH_EVAL_COST) {
    DgState st;
    if (int rc = dg_read_state(h, &st)) return rc;
    *out = st.f;
    return KMX_OK;
  }
  if (what == KMX_DGRAPH_EVAL_GRAD) {
    KMX_HIP(hipMemcpyAsync(out, d.b.get(), 6 * nn * sizeof(double), hipMemcpyDeviceToHost, s));
  } else if (what == KMX_DGRAPH_EVAL_BLOCKS) {
    KMX_HIP(hipMemcpyAsync(out, d.blk.get(), 21 * nn * sizeof(double), hipMemcpyDeviceToHost, s));
  } else {
    KMX_HIP(hipMemcpyAsync(d.p.get(), v, 6 * nn * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_dg_mask, dg_grid(n, 256), dim3(256), 0, s, n, d.mode.get(), d.p.get());
    const DgRec I{d.ptr.get(), d.other.get(), d.rec_w.get(), d.rec_d.get(), d.rec_a.get()};
    const DgPrior P{d.mode.get(), d.Rhat.get(), d.that.get(), d.kappa.get(), d.tau.get()};
    KMX_HIP(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL((k_dg_apply<true>), dim3(h->G.n_tiles), dim3(DG_TILE), 0, s, n, I, P, d.p.get(), d.q.get(),
                       d.st.get(), d.part.get());
    KMX_HIP(hipGetLastError());
    KMX_HIP(hipEventRecord(h->ev[1], s));
    KMX_HIP(hipMemcpyAsync(out, d.q.get(), 6 * nn * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  KMX_HIP(hipStreamSynchronize(s));
  if (what == KMX_DGRAPH_EVAL_JTJ) {
    float ms = 0.f;
    KMX_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[4] = ms;
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_solve(kmx_dgraph* h, const kmx_dgraph_params* params, kmx_dgraph_result* result) {
  KMX_GUARD_BEGIN
  kmx::DgParams Q;
  std::string err;
  if (int rc = kmx::dg_check_params(params, &Q, &err)) return kmx::fail(rc, "kmx_dgraph_solve: " + err);
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph && h->have_priors, KMX_ESTATE, "kmx_dgraph_solve before set_graph and set_priors");
  const int n = h->G.n, nt = h->G.n_tiles;
  h->log.clear();
  for (int k = 0; k < 4; ++k) h->ms[k] = 0.0;
  kmx_dgraph_result res{0.0, 0.0, Q.lambda_init, 0.0, 0, 0, 5, 0};
  if (n == 0) {
    if (result) *result = res;
    return KMX_OK;
  }
  KMX_HIP(hipSetDevice(h->device));
  DgDev& d = h->dev;
  hipStream_t s = h->stream;
  const DgRec I{d.ptr.get(), d.other.get(), d.rec_w.get(), d.rec_d.get(), d.rec_a.get()};
  const DgPrior P{d.mode.get(), d.Rhat.get(), d.that.get(), d.kappa.get(), d.tau.get()};
  const dim3 gt(nt), wave(DG_TILE), gn = dg_grid(n, 256), gn6 = dg_grid(6 * (int64_t)n, 256), b256(256), one(1);
  const double rtol2 = Q.cg_rtol * Q.cg_rtol;
  DgState st{};
  st.lambda = Q.lambda_init;
  KMX_HIP(hipMemcpyAsync(d.st.get(), &st, sizeof(st), hipMemcpyHostToDevice, s));
  KMX_HIP(hipEventRecord(h->ev[4], s));
  KMX_HIP(hipEventRecord(h->ev[0], s));
  if (int rc = dg_pin(h)) return rc;
  if (int rc = dg_linearize(h, 1)) return rc;
  if (int rc = dg_read_state(h, &st)) return rc;
  res.cost_initial = res.cost_final = st.f;
  res.gradnorm_initial = std::sqrt(st.bb);
  bool moved = false;  // the trial point was accepted and is not yet the current one
  if (st.bb == 0.0 || Q.max_iterations == 0) {
    res.stop_reason = st.bb == 0.0 ? 5 : 3;
  } else {
    for (int it = 0;; ++it) {
      if (it > 0) KMX_HIP(hipEventRecord(h->ev[0], s));
      if (moved) {
        KMX_HIP(hipMemcpyAsync(d.R.get(), d.Rt.get(), 9 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        KMX_HIP(hipMemcpyAsync(d.t.get(), d.tt.get(), 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        if (int rc = dg_linearize(h, 0)) return rc;
        moved = false;
      }
      hipLaunchKernelGGL(k_dg_precond, gn, b256, 0, s, n, d.mode.get(), d.blk.get(), d.st.get(), d.Minv.get());
      KMX_HIP(hipEventRecord(h->ev[1], s));
      hipLaunchKernelGGL(k_dg_cg_init, gt, wave, 0, s, n, d.b.get(), d.Minv.get(), d.x.get(), d.r.get(), d.z.get(),
                         d.p.get(), d.part.get());
      hipLaunchKernelGGL((k_dg_reduce<0>), one, wave, 0, s, d.part.get(), nt, d.st.get(), rtol2, Q.cg_max_iterations,
                         0);
      KMX_HIP(hipGetLastError());
      for (int done = 0; done < Q.cg_max_iterations;) {
        const int k = std::min(Q.check_every, Q.cg_max_iterations - done);
        for (int c = 0; c < k; ++c) {
          hipLaunchKernelGGL((k_dg_apply<false>), gt, wave, 0, s, n, I, P, d.p.get(), d.q.get(), d.st.get(),
                             d.part.get());
          hipLaunchKernelGGL((k_dg_reduce<1>), one, wave, 0, s, d.part.get(), nt, d.st.get(), rtol2,
                             Q.cg_max_iterations, 0);
          hipLaunchKernelGGL(k_dg_update, gt, wave, 0, s, n, d.Minv.get(), d.x.get(), d.r.get(), d.z.get(), d.p.get(),
                             d.q.get(), d.st.get(), d.part.get());
          hipLaunchKernelGGL((k_dg_reduce<2>), one, wave, 0, s, d.part.get(), nt, d.st.get(), rtol2,
                             Q.cg_max_iterations, 0);
          hipLaunchKernelGGL(k_dg_dir, gn6, b256, 0, s, 6 * n, d.z.get(), d.p.get(), d.st.get());
        }
        KMX_HIP(hipGetLastError());
        done += k;
        if (done >= Q.cg_max_iterations) break;
        int running = 0;
        KMX_HIP(hipMemcpyAsync(&running, &d.st.get()->cg_active, sizeof(int), hipMemcpyDeviceToHost, s));
        KMX_HIP(hipStreamSynchronize(s));
        if (!running) break;
      }
      KMX_HIP(hipEventRecord(h->ev[2], s));
      hipLaunchKernelGGL(k_dg_retract, gn, b256, 0, s, n, d.x.get(), d.R.get(), d.t.get(), d.Rt.get(), d.tt.get());
      hipLaunchKernelGGL((k_dg_linearize<false>), gt, wave, 0, s, n, I, P, d.Rt.get(), d.tt.get(), d.b.get(),
                         d.blk.get(), d.part.get());
      hipLaunchKernelGGL((k_dg_reduce<4>), one, wave, 0, s, d.part.get(), nt, d.st.get(), 0.0, 0, 0);
      hipLaunchKernelGGL(k_dg_decide, one, one, 0, s, d.st.get(), Q.factor, Q.lambda_min, Q.lambda_max, Q.rel_tol,
                         Q.abs_tol, Q.max_iterations);
      KMX_HIP(hipGetLastError());
      KMX_HIP(hipEventRecord(h->ev[3], s));
      const double f_before = st.f;
      if (int rc = dg_read_state(h, &st)) return rc;
      float a = 0.f, b = 0.f, c = 0.f;
      KMX_HIP(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
      KMX_HIP(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
      KMX_HIP(hipEventElapsedTime(&c, h->ev[2], h->ev[3]));
      h->ms[0] += a;
      h->ms[1] += b;
      h->ms[2] += c;
      h->log.push_back(kmx_dgraph_log_entry{f_before, st.f_trial, st.lambda_used, st.cg_iters, st.accepted});
      res.cg_iterations += st.cg_iters;
      moved = st.accepted != 0;
      if (st.stop) {
        res.stop_reason = st.stop;
        break;
      }
    }
    if (moved) {
      KMX_HIP(hipMemcpyAsync(d.R.get(), d.Rt.get(), 9 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
      KMX_HIP(hipMemcpyAsync(d.t.get(), d.tt.get(), 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
  }
  KMX_HIP(hipEventRecord(h->ev[5], s));
  KMX_HIP(hipStreamSynchronize(s));
  float tot = 0.f;
  KMX_HIP(hipEventElapsedTime(&tot, h->ev[4], h->ev[5]));
  h->ms[3] = tot;
  res.cost_final = st.f;
  res.lambda_final = st.lambda;
  res.iterations = st.iter;
  res.accepted = st.n_accepted;
  if (result) *result = res;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_dgraph_get_log(kmx_dgraph* h, int32_t cap, kmx_dgraph_log_entry* log, int32_t* n_out) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(cap >= 0 && (cap == 0 || log), KMX_EINVAL, "bad log buffer");
  const int32_t n = (int32_t)h->log.size();
  for (int32_t k = 0; k < std::min(cap, n); ++k) log[k] = h->log[(size_t)k];
  if (n_out) *n_out = n;
  return KMX_OK;
}

extern "C" int kmx_dgraph_get_timing(kmx_dgraph* h, double* ms) {
  KMX_CHECK(h && ms, KMX_EINVAL, "null argument");
  for (int k = 0; k < 5; ++k) ms[k] = h->ms[k];
  return KMX_OK;
}
