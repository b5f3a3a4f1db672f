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
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "chordal_host.h"
#include "common.h"

namespace {
using kmx::CH_TILE;

// One CG's scalars: a (block, row) of one stage.
struct ChScal {
  double bb, rr, rz, alpha, beta;
  int active, iters, conv, pad;
};

constexpr int CH_NPART = 9;  // partial sums per tile: up to 3 quantities x 3 rows

__device__ __forceinline__ double wave_sum(double v) {  // lane 0 holds the sum; fixed tree
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

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
                                                      const int* __restrict__ n_active, double* __restrict__ part) {
  constexpr int V = 3 * W;
  if (!INIT && *n_active == 0) return;
  const int tile = blockIdx.x, b = T.block[tile];
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
                                                  int max_it) {
  if (PHASE != 0 && *n_active == 0) return;
  const int b = blockIdx.x, lane = threadIdx.x;
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

__device__ inline void ch_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// A unit vector orthogonal to the unit vector u: the axis u is least along, made orthogonal.
__device__ inline void ch_any_orthogonal(const double* u, double* v) {
  int e = 0;
  if (fabs(u[1]) < fabs(u[e])) e = 1;
  if (fabs(u[2]) < fabs(u[e])) e = 2;
  double w[3] = {0.0, 0.0, 0.0};
  w[e] = 1.0;
  const double dot = u[e];
  double nn = 0.0;
  for (int k = 0; k < 3; ++k) {
    w[k] -= dot * u[k];
    nn += w[k] * w[k];
  }
  nn = sqrt(nn);
  for (int k = 0; k < 3; ++k) v[k] = w[k] / nn;
}

// v orthogonal to the unit vector u, and unit (one Gram-Schmidt step)
__device__ inline void ch_orthonormalize(const double* u, double* v) {
  double dot = 0.0, nn = 0.0;
  for (int k = 0; k < 3; ++k) dot += u[k] * v[k];
  for (int k = 0; k < 3; ++k) {
    v[k] -= dot * u[k];
    nn += v[k] * v[k];
  }
  nn = sqrt(nn);
  for (int k = 0; k < 3; ++k) v[k] /= nn;
}

// The nearest rotation to every free 3x3 block, as project_so3: with the SVD
// M = U S V^T, R = U diag(1, 1, det(U V^T)) V^T. One-sided Jacobi turns the
// columns of A = M V orthogonal (V a product of plane rotations); with u1, u2
// and v1, v2 the directions of the two largest singular values,
//   R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T,
// since det(U V^T) u3 v3^T = (u1 x u2)(v1 x v2)^T whatever the signs of u3 and
// v3: the determinant fix lands on the smallest singular direction and the
// smallest singular value is never divided by. A block of rank < 2 has no
// unique projection; the missing directions are completed so that the result
// is a rotation (the zero block gives I, as numpy's SVD does).
__global__ void k_ch_project(int n, const uint8_t* __restrict__ is_free, double* __restrict__ X) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !is_free[p]) return;
  double A[3][3], Vm[3][3];
  double amax = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      A[r][c] = X[(size_t)9 * p + 3 * r + c];
      Vm[r][c] = r == c ? 1.0 : 0.0;
      amax = fmax(amax, fabs(A[r][c]));
    }
  double Rm[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (amax > 0.0 && amax < INFINITY) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) A[r][c] /= amax;  // the projection does not depend on the scale
    for (int sweep = 0; sweep < 30; ++sweep) {
      bool rotated = false;
      for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j) {
          double aii = 0.0, ajj = 0.0, aij = 0.0;
          for (int r = 0; r < 3; ++r) {
            aii += A[r][i] * A[r][i];
            ajj += A[r][j] * A[r][j];
            aij += A[r][i] * A[r][j];
          }
          if (fabs(aij) <= 1e-17 * sqrt(aii * ajj) || aij == 0.0) continue;
          rotated = true;
          const double zeta = (ajj - aii) / (2.0 * aij);
          const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
          for (int r = 0; r < 3; ++r) {
            const double ai = A[r][i], aj = A[r][j];
            A[r][i] = cs * ai - sn * aj;
            A[r][j] = sn * ai + cs * aj;
            const double vi = Vm[r][i], vj = Vm[r][j];
            Vm[r][i] = cs * vi - sn * vj;
            Vm[r][j] = sn * vi + cs * vj;
          }
        }
      if (!rotated) break;
    }
    double s2[3];
    for (int c = 0; c < 3; ++c) s2[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c];
    int c1 = 0;
    if (s2[1] > s2[c1]) c1 = 1;
    if (s2[2] > s2[c1]) c1 = 2;
    int c2 = c1 == 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c)
      if (c != c1 && s2[c] > s2[c2]) c2 = c;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
    const double n1 = sqrt(s2[c1]);
    for (int r = 0; r < 3; ++r) {
      u1[r] = A[r][c1] / n1;
      v1[r] = Vm[r][c1];
    }
    if (s2[c2] > 1e-280) {
      const double n2 = sqrt(s2[c2]);
      for (int r = 0; r < 3; ++r) {
        u2[r] = A[r][c2] / n2;
        v2[r] = Vm[r][c2];
      }
      ch_orthonormalize(u1, u2);
      ch_orthonormalize(v1, v2);
    } else {
      ch_any_orthogonal(u1, u2);
      ch_any_orthogonal(v1, v2);
    }
    ch_cross(u1, u2, u3);
    ch_cross(v1, v2, v3);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Rm[r][c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) X[(size_t)9 * p + 3 * r + c] = Rm[r][c];
}

struct ChDev {  // what set_graph puts on the device
  int *tile_p0 = nullptr, *tile_p1 = nullptr, *tile_block = nullptr, *tile_ptr = nullptr, *inc_ptr = nullptr;
  uint32_t* inc_other = nullptr;
  double *inc_M = nullptr, *inc_t = nullptr, *wk = nullptr, *wt = nullptr;
  uint8_t* is_free = nullptr;
  double *Dk = nullptr, *Dt = nullptr, *xr = nullptr, *xt = nullptr, *r = nullptr, *d = nullptr, *q = nullptr,
         *bt = nullptr, *part = nullptr;
  ChScal* sc = nullptr;  // [2][3 nb]: rotations, translations
  int* ctl = nullptr;    // [2] (block, row) pairs still running, per stage
  int n_tiles = 0;
};

void ch_free(ChDev& d) {
  void* ptrs[] = {d.tile_p0, d.tile_p1, d.tile_block, d.tile_ptr, d.inc_ptr, d.inc_other, d.inc_M, d.inc_t,
                  d.wk, d.wt, d.is_free, d.Dk, d.Dt, d.xr, d.xt, d.r, d.d, d.q, d.bt, d.part, d.sc, d.ctl};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  d = ChDev();
}

template <class T>
int ch_alloc(T** p, size_t count) {
  if (hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
    *p = nullptr;
    return kmx::fail(KMX_ENOMEM, "hipMalloc failed");
  }
  return KMX_OK;
}

template <class T>
int ch_put(T** p, const std::vector<T>& v, hipStream_t s) {
  if (int rc = ch_alloc(p, v.size())) return rc;
  if (!v.empty()) KMX_HIP(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return KMX_OK;
}

}  // namespace

struct kmx_chordal {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool have_graph = false;
  kmx::ChordalGraph g;
  ChDev dev;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool timed = false;
};

namespace {

int ch_upload_weights(kmx_chordal* h, ChDev& d, const kmx::ChordalGraph& g, const double* weight) {
  std::vector<double> wk, wt;
  kmx::chordal_record_weights(g, weight, &wk, &wt);
  if (!wk.empty()) {
    KMX_HIP(hipMemcpyAsync(d.wk, wk.data(), wk.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(d.wt, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(k_ch_diag, dim3((g.n + 255) / 256), dim3(256), 0, h->stream, g.n, d.inc_ptr, d.wk, d.wt, d.Dk,
                     d.Dt);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipStreamSynchronize(h->stream));  // wk / wt are host temporaries
  return KMX_OK;
}

// One stage: the start (residual, who runs), then CG in batches of
// check_every iterations until the device says nobody runs, at most max_it.
template <int W>
int ch_stage(kmx_chordal* h, int stage, double* x, const double* rhs, double rtol, int max_it, int check_every) {
  ChDev& d = h->dev;
  const kmx::ChordalGraph& g = h->g;
  hipStream_t s = h->stream;
  const ChTiles T{d.tile_p0, d.tile_p1, d.tile_block};
  const ChInc I{d.inc_ptr, d.inc_other, W == 3 ? d.wk : d.wt, d.inc_M};
  const double* D = W == 3 ? d.Dk : d.Dt;
  ChScal* sc = d.sc + (size_t)stage * 3 * g.nb;
  int* ctl = d.ctl + stage;
  const double rtol2 = rtol * rtol;
  const dim3 gt(d.n_tiles), gb(g.nb), wave(CH_TILE);
  KMX_HIP(hipMemsetAsync(ctl, 0, sizeof(int), s));
  hipLaunchKernelGGL((k_ch_apply<W, true>), gt, wave, 0, s, T, I, d.is_free, D, x, rhs, d.r, d.d, sc, ctl, d.part);
  hipLaunchKernelGGL((k_ch_reduce<0>), gb, wave, 0, s, d.tile_ptr, d.part, sc, ctl, rtol2, max_it);
  KMX_HIP(hipGetLastError());
  for (int done = 0; done < max_it;) {
    int running = 0;
    KMX_HIP(hipMemcpyAsync(&running, ctl, sizeof(int), hipMemcpyDeviceToHost, s));
    KMX_HIP(hipStreamSynchronize(s));
    if (running == 0) break;
    const int k = std::min(check_every, max_it - done);
    for (int it = 0; it < k; ++it) {
      hipLaunchKernelGGL((k_ch_apply<W, false>), gt, wave, 0, s, T, I, d.is_free, D, d.d, nullptr, d.q, nullptr, sc,
                         ctl, d.part);
      hipLaunchKernelGGL((k_ch_reduce<1>), gb, wave, 0, s, d.tile_ptr, d.part, sc, ctl, rtol2, max_it);
      hipLaunchKernelGGL((k_ch_update<W>), gt, wave, 0, s, T, d.is_free, D, x, d.r, d.d, d.q, sc, ctl, d.part);
      hipLaunchKernelGGL((k_ch_reduce<2>), gb, wave, 0, s, d.tile_ptr, d.part, sc, ctl, rtol2, max_it);
      hipLaunchKernelGGL((k_ch_dir<W>), gt, wave, 0, s, T, d.is_free, D, d.r, d.d, sc, ctl);
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
  int ndev = 0;
  KMX_HIP(hipGetDeviceCount(&ndev));
  KMX_CHECK(device >= 0 && device < ndev, KMX_EINVAL, "bad HIP device ordinal");
  KMX_HIP(hipSetDevice(device));
  kmx_chordal* h = new kmx_chordal();
  h->device = device;
  bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
  h->own_stream = ok;
  for (int k = 0; ok && k < 5; ++k) ok = hipEventCreate(&h->ev[k]) == hipSuccess;
  if (!ok) {
    for (hipEvent_t e : h->ev)
      if (e) (void)hipEventDestroy(e);
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return kmx::fail(KMX_EHIP, "hipStreamCreate / hipEventCreate failed");
  }
  *out = h;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_chordal_destroy(kmx_chordal* h) {
  if (!h) return KMX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  ch_free(h->dev);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return KMX_OK;
}

extern "C" int kmx_chordal_set_stream(kmx_chordal* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  if (h->stream) KMX_HIP(hipStreamSynchronize(h->stream));
  if (h->own_stream && h->stream) KMX_HIP(hipStreamDestroy(h->stream));
  h->own_stream = false;
  h->stream = reinterpret_cast<hipStream_t>(s);
  return KMX_OK;
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
  ChDev d;
  d.n_tiles = (int)g.tile_p0.size();
  const size_t n = (size_t)g.n, nrec = g.inc_other.size();
  int rc = KMX_OK;
  if ((rc = ch_put(&d.tile_p0, g.tile_p0, s)) || (rc = ch_put(&d.tile_p1, g.tile_p1, s)) ||
      (rc = ch_put(&d.tile_block, g.tile_block, s)) || (rc = ch_put(&d.tile_ptr, g.tile_ptr, s)) ||
      (rc = ch_put(&d.inc_ptr, g.inc_ptr, s)) || (rc = ch_put(&d.inc_other, g.inc_other, s)) ||
      (rc = ch_put(&d.inc_M, g.inc_M, s)) || (rc = ch_put(&d.inc_t, g.inc_t, s)) ||
      (rc = ch_put(&d.is_free, g.is_free, s)) || (rc = ch_alloc(&d.wk, nrec)) || (rc = ch_alloc(&d.wt, nrec)) ||
      (rc = ch_alloc(&d.Dk, n)) || (rc = ch_alloc(&d.Dt, n)) || (rc = ch_alloc(&d.xr, 9 * n)) ||
      (rc = ch_alloc(&d.xt, 3 * n)) || (rc = ch_alloc(&d.r, 9 * n)) || (rc = ch_alloc(&d.d, 9 * n)) ||
      (rc = ch_alloc(&d.q, 9 * n)) || (rc = ch_alloc(&d.bt, 3 * n)) ||
      (rc = ch_alloc(&d.part, (size_t)CH_NPART * d.n_tiles)) || (rc = ch_alloc(&d.sc, (size_t)6 * g.nb)) ||
      (rc = ch_alloc(&d.ctl, 2)) || (rc = ch_upload_weights(h, d, g, weight))) {
    (void)hipStreamSynchronize(s);
    ch_free(d);
    return rc;
  }
  // the incidence arrays are only read on the device from here on; the host
  // keeps what set_weights needs
  g.inc_M = std::vector<double>();
  g.inc_t = std::vector<double>();
  ch_free(h->dev);
  h->dev = d;
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
  return ch_upload_weights(h, h->dev, g, weight);
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
  KMX_HIP(hipMemcpyAsync(d.xr, xr.data(), 9 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipMemcpyAsync(d.xt, xt.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipEventRecord(h->ev[1], s));
  int rc = ch_stage<3>(h, 0, d.xr, nullptr, rtol, max_it, check_every);
  if (rc) return rc;
  const dim3 gp((g.n + 255) / 256), bp(256);
  hipLaunchKernelGGL(k_ch_project, gp, bp, 0, s, g.n, d.is_free, d.xr);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipEventRecord(h->ev[2], s));
  hipLaunchKernelGGL(k_ch_rhs_t, gp, bp, 0, s, g.n, d.inc_ptr, d.inc_other, d.wt, d.inc_t, d.is_free, d.xr, d.bt);
  KMX_HIP(hipGetLastError());
  rc = ch_stage<1>(h, 1, d.xt, d.bt, rtol, max_it, check_every);
  if (rc) return rc;
  KMX_HIP(hipEventRecord(h->ev[3], s));
  std::vector<ChScal> sc((size_t)6 * g.nb);
  KMX_HIP(hipMemcpyAsync(R_out, d.xr, 9 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(t_out, d.xt, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipMemcpyAsync(sc.data(), d.sc, sc.size() * sizeof(ChScal), hipMemcpyDeviceToHost, s));
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
