// cert.hip — kmx_cert_*: the dual optimality certificate of an RBCD solution
// (DESIGN.md §16): lambda_min of S(X) = Q - Lambda(X) by plain
// Lanczos on the device.
//
// The graph is the team graph, poses flattened to 0..n-1. A lane owns a pose;
// a tile is 64 consecutive poses (one wave). kmx_cert_set_point forms the
// symmetric 4x4 D_i - Lambda_i of every pose (10 doubles); S v is then one pass
// over the incidence records: a 128-byte record per incidence (R, t, w kappa,
// w tau, the other endpoint with the role flag) plus the other endpoint's
// 32-byte row of v. A tail record applies C = [[kappa R, tau t], [0, tau]], a
// head record applies C^T.
//
// A Lanczos step is k_ct_apply (w = S v - beta v_prev, tile partials of
// <v, w>), k_ct_reduce (alpha), k_ct_update (w -= alpha v, partials of |w|^2),
// k_ct_reduce (beta). The vectors are kept unnormalised: the division by beta
// is folded into the next apply. alpha_j and beta_j go to device arrays; the
// host enqueues check_every steps, reads the new coefficients and applies the
// rule (cert_host.h) at multiples of test_every, so check_every changes no bit.
// Sums are ordered: a pose adds its records in the CSR's order, a tile reduces
// with a fixed shuffle tree, one wave sums the tile partials in a fixed order.
// No floating-point atomics, no grid barrier, no persistent kernel, no
// device-side wait.
//
// The escape step of the Riemannian staircase lives here too:
// kmx_cert_escape lifts the point to rank r + 1 along a direction y for up to 8
// step lengths (k_ct_lift) and evaluates each candidate's cost (k_ct_cost, the
// candidate on blockIdx.y; k_ct_reduce sums the tile partials of all of them),
// kmx_cert_escape_commit makes one of them the point without an upload.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "cert_host.h"
#include "common.h"

namespace {
using kmx::CT_TILE;

// One incidence: 128 bytes, read whole by the lane that owns the pose.
struct alignas(16) CtRec {
  double R[9];
  double t[3];
  double wk, wt;  // w kappa, w tau (both 0: the edge is dropped)
  uint32_t other; // other endpoint | CT_TAIL
  uint32_t pad0;
  double pad1;
};
static_assert(sizeof(CtRec) == 128, "incidence record is 128 bytes");

using kmx::wave_sum;  // lane 0 holds the sum; fixed tree

// y = M x for the symmetric 4x4 packed as (00 01 02 03 11 12 13 22 23 33)
__device__ __forceinline__ void ct_sym4(const double* m, const double* x, double* y) {
  y[0] = m[0] * x[0] + m[1] * x[1] + m[2] * x[2] + m[3] * x[3];
  y[1] = m[1] * x[0] + m[4] * x[1] + m[5] * x[2] + m[6] * x[3];
  y[2] = m[2] * x[0] + m[5] * x[1] + m[7] * x[2] + m[8] * x[3];
  y[3] = m[3] * x[0] + m[6] * x[1] + m[8] * x[2] + m[9] * x[3];
}

// acc -= w C x (tail) or w C^T x (head), x and acc rows of 4
__device__ __forceinline__ void ct_edge(const CtRec& e, bool tail, const double* x, double* acc) {
  if (tail) {
    for (int c = 0; c < 3; ++c)
      acc[c] -= e.wk * (e.R[3 * c] * x[0] + e.R[3 * c + 1] * x[1] + e.R[3 * c + 2] * x[2]) + e.wt * e.t[c] * x[3];
    acc[3] -= e.wt * x[3];
  } else {
    for (int c = 0; c < 3; ++c) acc[c] -= e.wk * (e.R[c] * x[0] + e.R[3 + c] * x[1] + e.R[6 + c] * x[2]);
    acc[3] -= e.wt * (e.t[0] * x[0] + e.t[1] * x[1] + e.t[2] * x[2] + x[3]);
  }
}

// The point: per pose D (the diagonal block of Q, from its records), G = (X Q)_p,
// Lambda = sym(Y^T G_Y), Dm = D - Lambda, and the tile partials of tr(X Q X^T),
// tr Lambda and |X S|_F^2 with (X S)_p = G - X_p [Lambda 0; 0 0].
template <int R>
__global__ __launch_bounds__(CT_TILE) void k_ct_point(int n, const int* __restrict__ ptr,
                                                      const CtRec* __restrict__ rec, const double* __restrict__ X,
                                                      double* __restrict__ Dm, double* __restrict__ Lam,
                                                      double* __restrict__ part) {
  const int p = blockIdx.x * CT_TILE + (int)threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  if (p < n) {
    double x[R][4], g[R][4], D[10];
    for (int a = 0; a < R; ++a)
      for (int c = 0; c < 4; ++c) {
        x[a][c] = X[((size_t)p * R + a) * 4 + c];
        g[a][c] = 0.0;
      }
    for (int k = 0; k < 10; ++k) D[k] = 0.0;
    const int k1 = ptr[p + 1];
    for (int k = ptr[p]; k < k1; ++k) {
      const CtRec e = rec[k];
      if (e.wk == 0.0 && e.wt == 0.0) continue;
      const bool tail = (e.other & kmx::CT_TAIL) != 0;
      const int o = (int)(e.other & 0x7fffffffu);
      if (tail) {
        D[0] += e.wk + e.wt * e.t[0] * e.t[0];
        D[1] += e.wt * e.t[0] * e.t[1];
        D[2] += e.wt * e.t[0] * e.t[2];
        D[3] += e.wt * e.t[0];
        D[4] += e.wk + e.wt * e.t[1] * e.t[1];
        D[5] += e.wt * e.t[1] * e.t[2];
        D[6] += e.wt * e.t[1];
        D[7] += e.wk + e.wt * e.t[2] * e.t[2];
        D[8] += e.wt * e.t[2];
        D[9] += e.wt;
      } else {
        D[0] += e.wk;
        D[4] += e.wk;
        D[7] += e.wk;
        D[9] += e.wt;
      }
      for (int a = 0; a < R; ++a) {
        double xo[4];
        for (int c = 0; c < 4; ++c) xo[c] = X[((size_t)o * R + a) * 4 + c];
        ct_edge(e, tail, xo, g[a]);
      }
    }
    for (int a = 0; a < R; ++a) {
      double y[4];
      ct_sym4(D, x[a], y);
      for (int c = 0; c < 4; ++c) g[a][c] += y[c];
    }
    double L[3][3];
    for (int c = 0; c < 3; ++c)
      for (int d = c; d < 3; ++d) {
        double v = 0.0;
        for (int a = 0; a < R; ++a) v += x[a][c] * g[a][d] + x[a][d] * g[a][c];
        L[c][d] = L[d][c] = 0.5 * v;
      }
    for (int c = 0; c < 3; ++c)
      for (int d = 0; d < 3; ++d) Lam[(size_t)9 * p + 3 * c + d] = L[c][d];
    double* dm = Dm + (size_t)10 * p;
    dm[0] = D[0] - L[0][0];
    dm[1] = D[1] - L[0][1];
    dm[2] = D[2] - L[0][2];
    dm[3] = D[3];
    dm[4] = D[4] - L[1][1];
    dm[5] = D[5] - L[1][2];
    dm[6] = D[6];
    dm[7] = D[7] - L[2][2];
    dm[8] = D[8];
    dm[9] = D[9];
    s[1] = L[0][0] + L[1][1] + L[2][2];
    for (int a = 0; a < R; ++a) {
      for (int c = 0; c < 4; ++c) s[0] += x[a][c] * g[a][c];
      for (int c = 0; c < 3; ++c) {
        const double q = g[a][c] - (x[a][0] * L[0][c] + x[a][1] * L[1][c] + x[a][2] * L[2][c]);
        s[2] += q * q;
      }
      s[2] += g[a][3] * g[a][3];
    }
  }
  for (int q = 0; q < 3; ++q) {
    const double v = wave_sum(s[q]);
    if (threadIdx.x == 0) part[(size_t)3 * blockIdx.x + q] = v;
  }
}

// w = S v - beta v_prev with v = u / B[j], v_prev = u_prev / B[j-1] and
// beta = B[j] (B[0] = |u_0|, B[j+1] = beta_j; u, u_prev: the unnormalised
// vectors), and the tile partial of <v, w>. B == NULL: out = S u (caller data).
__global__ __launch_bounds__(CT_TILE) void k_ct_apply(int n, const int* __restrict__ ptr,
                                                      const CtRec* __restrict__ rec, const double* __restrict__ Dm,
                                                      const double* __restrict__ u, const double* __restrict__ uprev,
                                                      const double* __restrict__ B, int j, double* __restrict__ out,
                                                      double* __restrict__ part) {
  const int p = blockIdx.x * CT_TILE + (int)threadIdx.x;
  const double inv = B ? 1.0 / B[j] : 1.0;
  const double cprev = (B && j > 0) ? B[j] / B[j - 1] : 0.0;
  double s = 0.0;
  if (p < n) {
    double v[4], acc[4], dm[10];
    for (int c = 0; c < 4; ++c) v[c] = u[(size_t)4 * p + c] * inv;
    for (int k = 0; k < 10; ++k) dm[k] = Dm[(size_t)10 * p + k];
    ct_sym4(dm, v, acc);
    const int k1 = ptr[p + 1];
    for (int k = ptr[p]; k < k1; ++k) {
      const CtRec e = rec[k];
      if (e.wk == 0.0 && e.wt == 0.0) continue;
      const int o = (int)(e.other & 0x7fffffffu);
      double vo[4];
      for (int c = 0; c < 4; ++c) vo[c] = u[(size_t)4 * o + c] * inv;
      ct_edge(e, (e.other & kmx::CT_TAIL) != 0, vo, acc);
    }
    for (int c = 0; c < 4; ++c) {
      double w = acc[c];
      if (cprev != 0.0) w -= cprev * uprev[(size_t)4 * p + c];
      out[(size_t)4 * p + c] = w;
      s += v[c] * w;
    }
  }
  if (part) {
    const double t = wave_sum(s);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
  }
}

// The tile partials (nq per tile), summed by one wave in a fixed order (lane l
// takes tiles l, l + 64, ... in turn, then the shuffle tree); root: the square
// root of the sum (a norm).
__global__ __launch_bounds__(64) void k_ct_reduce(int n_tiles, int nq, const double* __restrict__ part,
                                                  double* __restrict__ out, int root) {
  const int lane = threadIdx.x;
  for (int q = 0; q < nq; ++q) {
    double v = 0.0;
    for (int t = lane; t < n_tiles; t += 64) v += part[(size_t)nq * t + q];
    v = wave_sum(v);
    if (lane == 0) out[q] = root ? sqrt(v) : v;
  }
}

// w -= alpha v (v = u / B[j]) and the tile partial of |w|^2; ACC (the vector
// pass): y += s_j v too.
template <bool ACC>
__global__ __launch_bounds__(CT_TILE) void k_ct_update(int n, const double* __restrict__ u,
                                                       const double* __restrict__ B, const double* __restrict__ alpha,
                                                       int j, double* __restrict__ w, double* __restrict__ part,
                                                       const double* __restrict__ sv, double* __restrict__ y) {
  const int p = blockIdx.x * CT_TILE + (int)threadIdx.x;
  const double inv = 1.0 / B[j], a = alpha[j];
  double s = 0.0;
  if (p < n) {
    const double sj = ACC ? sv[j] : 0.0;
    for (int c = 0; c < 4; ++c) {
      const size_t k = (size_t)4 * p + c;
      const double v = u[k] * inv;
      const double r = w[k] - a * v;
      w[k] = r;
      s += r * r;
      if (ACC) y[k] += sj * v;
    }
  }
  const double t = wave_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// The tile partials of |u|^2 (the start vector's norm).
__global__ __launch_bounds__(CT_TILE) void k_ct_norm2(int n, const double* __restrict__ u, double* __restrict__ part) {
  const int p = blockIdx.x * CT_TILE + (int)threadIdx.x;
  double s = 0.0;
  if (p < n)
    for (int c = 0; c < 4; ++c) s += u[(size_t)4 * p + c] * u[(size_t)4 * p + c];
  const double t = wave_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// The records' w kappa and w tau from the interleaved upload [rec][2].
__global__ void k_ct_weights(int64_t nrec, const double* __restrict__ wkt, CtRec* __restrict__ rec) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nrec) return;
  rec[k].wk = wkt[2 * k];
  rec[k].wt = wkt[2 * k + 1];
}

// The escape step's candidates: candidate blockIdx.y of pose p
// is [X_p; a y_p^T] (R + 1 rows of 4) with a = alpha[blockIdx.y], its three
// rotation columns orthonormalised by Gram-Schmidt in column order, every
// column projected twice against the ones before it and then divided by its
// norm (a positive diagonal). The translation column passes through. A pose
// whose new rotation entries are all zero (a = 0, or y_p has none) is copied:
// its X_p is on the manifold as it stands. cand is [n_alpha][n][R + 1][4].
template <int R>
__global__ __launch_bounds__(CT_TILE) void k_ct_lift(int n, const double* __restrict__ X,
                                                     const double* __restrict__ y,
                                                     const double* __restrict__ alpha, double* __restrict__ cand) {
  const int p = blockIdx.x * CT_TILE + (int)threadIdx.x;
  if (p >= n) return;
  const double a = alpha[blockIdx.y];
  double z[R + 1][4];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) z[i][c] = X[((size_t)p * R + i) * 4 + c];
#pragma unroll
  for (int c = 0; c < 4; ++c) z[R][c] = a * y[(size_t)4 * p + c];
  if (z[R][0] != 0.0 || z[R][1] != 0.0 || z[R][2] != 0.0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int d = 0; d < c; ++d) {
          double dot = 0.0;
#pragma unroll
          for (int i = 0; i <= R; ++i) dot += z[i][d] * z[i][c];
#pragma unroll
          for (int i = 0; i <= R; ++i) z[i][c] -= dot * z[i][d];
        }
      double nn = 0.0;
#pragma unroll
      for (int i = 0; i <= R; ++i) nn += z[i][c] * z[i][c];
      const double nrm = sqrt(nn);
      if (nrm > 0.0) {
#pragma unroll
        for (int i = 0; i <= R; ++i) z[i][c] /= nrm;
      }
    }
  }
  double* out = cand + (((size_t)blockIdx.y * n + p) * (R + 1)) * 4;
#pragma unroll
  for (int i = 0; i <= R; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4 * i + c] = z[i][c];
}

// The tile partials of tr(Z Q Z^T) = sum_p <Z_p, (Z Q)_p> for candidate
// blockIdx.y (Z = cand + blockIdx.y n R 4, rank R): D_p and (Z Q)_p from the
// pose's records as k_ct_point forms them, in the CSR's order.
// part is [tile][n_alpha], the layout k_ct_reduce sums.
template <int R>
__global__ __launch_bounds__(CT_TILE) void k_ct_cost(int n, const int* __restrict__ ptr,
                                                     const CtRec* __restrict__ rec, const double* __restrict__ cand,
                                                     double* __restrict__ part) {
  const int p = blockIdx.x * CT_TILE + (int)threadIdx.x;
  const double* __restrict__ Z = cand + (size_t)blockIdx.y * n * R * 4;
  double s = 0.0;
  if (p < n) {
    double x[R][4], g[R][4], D[10];
    for (int a = 0; a < R; ++a)
      for (int c = 0; c < 4; ++c) {
        x[a][c] = Z[((size_t)p * R + a) * 4 + c];
        g[a][c] = 0.0;
      }
    for (int k = 0; k < 10; ++k) D[k] = 0.0;
    const int k1 = ptr[p + 1];
    for (int k = ptr[p]; k < k1; ++k) {
      const CtRec e = rec[k];
      if (e.wk == 0.0 && e.wt == 0.0) continue;
      const bool tail = (e.other & kmx::CT_TAIL) != 0;
      const int o = (int)(e.other & 0x7fffffffu);
      if (tail) {
        D[0] += e.wk + e.wt * e.t[0] * e.t[0];
        D[1] += e.wt * e.t[0] * e.t[1];
        D[2] += e.wt * e.t[0] * e.t[2];
        D[3] += e.wt * e.t[0];
        D[4] += e.wk + e.wt * e.t[1] * e.t[1];
        D[5] += e.wt * e.t[1] * e.t[2];
        D[6] += e.wt * e.t[1];
        D[7] += e.wk + e.wt * e.t[2] * e.t[2];
        D[8] += e.wt * e.t[2];
        D[9] += e.wt;
      } else {
        D[0] += e.wk;
        D[4] += e.wk;
        D[7] += e.wk;
        D[9] += e.wt;
      }
      for (int a = 0; a < R; ++a) {
        double xo[4];
        for (int c = 0; c < 4; ++c) xo[c] = Z[((size_t)o * R + a) * 4 + c];
        ct_edge(e, tail, xo, g[a]);
      }
    }
    for (int a = 0; a < R; ++a) {
      double v[4];
      ct_sym4(D, x[a], v);
      for (int c = 0; c < 4; ++c) s += x[a][c] * (g[a][c] + v[c]);
    }
  }
  const double t = wave_sum(s);
  if (threadIdx.x == 0) part[(size_t)gridDim.y * blockIdx.x + blockIdx.y] = t;
}

struct CtDev {  // what set_graph puts on the device; replaced as a whole
  kmx::DevBuf<int> ptr;
  kmx::DevBuf<CtRec> rec;
  kmx::DevBuf<double> wkt, X, Dm, Lam, part, scal;
  kmx::DevBuf<double> vec[3];
  kmx::DevBuf<double> y;
  // min_eig's coefficients, max_steps + 1 each, allocated by its first call and regrown together (sv last)
  kmx::DevBuf<double> alpha, B, sv;
  // the escape step: the candidates [n_alpha][n][r + 1][4] (grown on demand), the tile partials
  // [n_tiles][CT_MAX_ALPHA], and the step lengths [0..7] with the costs [8..15]
  kmx::DevBuf<double> cand, epart, esc;
};

enum { EV_POINT0, EV_POINT1, EV_A, EV_B, EV_C, EV_D, EV_COUNT };  // EV_A..EV_D: min_eig's, and escape's

}  // namespace

struct kmx_cert : kmx::StreamCore {
  bool have_graph = false, have_point = false;
  int r = 0;
  kmx::CertGraph g;
  CtDev dev;
  kmx::Event ev[EV_COUNT];
  bool timed_point = false;
  // the last min_eig's: device ms of the Lanczos steps, of the vector pass, of the transfers (HIP events,
  // summed over the batches), and host ms of the decisions and of the whole call (the host clock)
  double ms_lan = 0.0, ms_vec = 0.0, ms_xfer = 0.0, ms_host_rule = 0.0, ms_host_wall = 0.0;
  std::vector<double> alpha, beta;  // the last min_eig's, as far as the host read them
  // the escape step: the point's cost (set_point's, kept for the choice rule), and the candidates of the last
  // kmx_cert_escape while they are valid (n_esc > 0: their count, for the point of rank r)
  double cost = 0.0;
  int n_esc = 0;
  double ms_esc = 0.0, ms_esc_xfer = 0.0;  // the last escape's kernels and transfers (HIP events)
};

namespace {

int ct_upload_weights(kmx_cert* h, CtDev& d, const kmx::CertGraph& g, const double* weight) {
  std::vector<double> wkt;
  kmx::cert_record_weights(g, weight, &wkt);
  const int64_t nrec = (int64_t)g.inc_edge.size();
  if (nrec > 0) {
    KMX_HIP(hipMemcpyAsync(d.wkt.get(), wkt.data(), wkt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_ct_weights, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, h->stream, nrec, d.wkt.get(),
                       d.rec.get());
    KMX_HIP(hipGetLastError());
  }
  KMX_HIP(hipStreamSynchronize(h->stream));  // wkt is a host temporary
  return KMX_OK;
}

// The point kernel and its three sums (cost, tr Lambda, |X S|_F^2) to d.scal.
int ct_run_point(kmx_cert* h) {
  CtDev& d = h->dev;
  const kmx::CertGraph& g = h->g;
  const dim3 gt(g.n_tiles), wave(CT_TILE);
  hipStream_t s = h->stream;
#define KMX_CT_POINT(RR)                                                                                       \
  case RR:                                                                                                     \
    hipLaunchKernelGGL((k_ct_point<RR>), gt, wave, 0, s, g.n, d.ptr.get(), d.rec.get(), d.X.get(), d.Dm.get(), \
                       d.Lam.get(), d.part.get());                                                             \
    break;
  switch (h->r) {
    KMX_CT_POINT(3)
    KMX_CT_POINT(4)
    KMX_CT_POINT(5)
    KMX_CT_POINT(6)
    KMX_CT_POINT(7)
    KMX_CT_POINT(8)
    default:
      return kmx::fail(KMX_EINVAL, "r outside 3..8");
  }
#undef KMX_CT_POINT
  hipLaunchKernelGGL(k_ct_reduce, dim3(1), dim3(64), 0, s, g.n_tiles, 3, d.part.get(), d.scal.get(), 0);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

// Steps j0 .. j0 + k - 1; vec[j % 3] holds u_j. ACC: the vector pass.
template <bool ACC>
void ct_enqueue_steps(kmx_cert* h, int j0, int k) {
  CtDev& d = h->dev;
  const kmx::CertGraph& g = h->g;
  const dim3 gt(g.n_tiles), wave(CT_TILE);
  hipStream_t s = h->stream;
  for (int j = j0; j < j0 + k; ++j) {
    const double* u = d.vec[j % 3].get();
    const double* up = d.vec[(j + 2) % 3].get();
    double* w = d.vec[(j + 1) % 3].get();
    hipLaunchKernelGGL(k_ct_apply, gt, wave, 0, s, g.n, d.ptr.get(), d.rec.get(), d.Dm.get(), u, up, d.B.get(), j, w,
                       d.part.get());
    hipLaunchKernelGGL(k_ct_reduce, dim3(1), dim3(64), 0, s, g.n_tiles, 1, d.part.get(), d.alpha.get() + j, 0);
    hipLaunchKernelGGL((k_ct_update<ACC>), gt, wave, 0, s, g.n, u, d.B.get(), d.alpha.get(), j, w, d.part.get(),
                       d.sv.get(), d.y.get());
    hipLaunchKernelGGL(k_ct_reduce, dim3(1), dim3(64), 0, s, g.n_tiles, 1, d.part.get(), d.B.get() + j + 1, 1);
  }
}

// The norm of the start vector in vec[0] to B[0].
int ct_start_norm(kmx_cert* h) {
  CtDev& d = h->dev;
  const kmx::CertGraph& g = h->g;
  hipStream_t s = h->stream;
  hipLaunchKernelGGL(k_ct_norm2, dim3(g.n_tiles), dim3(CT_TILE), 0, s, g.n, d.vec[0].get(), d.part.get());
  hipLaunchKernelGGL(k_ct_reduce, dim3(1), dim3(64), 0, s, g.n_tiles, 1, d.part.get(), d.B.get(), 1);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

// ms between two events of the handle that have completed, added to *acc.
int ct_span(kmx_cert* h, int a, int b, double* acc) {
  float t = 0.f;
  KMX_HIP(hipEventElapsedTime(&t, h->ev[a], h->ev[b]));
  *acc += t;
  return KMX_OK;
}

double ct_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" int kmx_cert_create(int device, kmx_cert** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  std::unique_ptr<kmx_cert> h(new kmx_cert());
  int rc;
  if ((rc = h->open(device)) || (rc = kmx::create_events(h->ev))) return rc;
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_destroy(kmx_cert* h) {
  return kmx::destroy(h);
}

extern "C" int kmx_cert_set_stream(kmx_cert* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, true);
}

extern "C" int kmx_cert_set_graph(kmx_cert* h, int32_t n_poses, int64_t n_edges, const int32_t* src,
                                  const int32_t* dst, const double* R, const double* t, const double* kappa,
                                  const double* tau, const double* weight) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  kmx::CertGraph g;
  std::string err;
  if (kmx::cert_build(n_poses, n_edges, src, dst, R, t, kappa, tau, weight, &g, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_cert_set_graph: " + err);
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  hipStream_t s = h->stream;
  const size_t n = (size_t)g.n, nrec = g.inc_other.size();
  std::vector<CtRec> recs(nrec);
  for (size_t k = 0; k < nrec; ++k) {
    const int32_t e = g.inc_edge[k];
    CtRec& c = recs[k];
    std::memcpy(c.R, R + (size_t)9 * e, 9 * sizeof(double));
    std::memcpy(c.t, t + (size_t)3 * e, 3 * sizeof(double));
    c.wk = c.wt = 0.0;
    c.other = g.inc_other[k];
    c.pad0 = 0;
    c.pad1 = 0.0;
  }
  // built aside, committed by the move below: an error or an exception on its way to KMX_GUARD_END frees only d
  CtDev d;
  int rc = KMX_OK;
  if ((rc = d.ptr.alloc(n + 1)) || (rc = d.rec.alloc(nrec)) || (rc = d.wkt.alloc(2 * nrec)) ||
      (rc = d.X.alloc(n * 32)) || (rc = d.Dm.alloc(n * 10)) || (rc = d.Lam.alloc(n * 9)) ||
      (rc = d.part.alloc((size_t)3 * g.n_tiles)) || (rc = d.scal.alloc(4)) || (rc = d.vec[0].alloc(4 * n)) ||
      (rc = d.vec[1].alloc(4 * n)) || (rc = d.vec[2].alloc(4 * n)) || (rc = d.y.alloc(4 * n)) ||
      (rc = d.epart.alloc((size_t)kmx::CT_MAX_ALPHA * g.n_tiles)) || (rc = d.esc.alloc(2 * (size_t)kmx::CT_MAX_ALPHA)))
    return rc;
  hipError_t e1 = hipMemcpyAsync(d.ptr.get(), g.inc_ptr.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice, s);
  hipError_t e2 = nrec ? hipMemcpyAsync(d.rec.get(), recs.data(), nrec * sizeof(CtRec), hipMemcpyHostToDevice, s)
                       : hipSuccess;
  if (e1 != hipSuccess || e2 != hipSuccess || (rc = ct_upload_weights(h, d, g, weight))) {
    (void)hipStreamSynchronize(s);  // the uploads read g and recs
    return rc ? rc : kmx::fail(KMX_EHIP, "hipMemcpyAsync failed");
  }
  h->dev = std::move(d);
  h->g = std::move(g);
  h->have_graph = true;
  h->have_point = false;
  h->timed_point = false;
  h->n_esc = 0;
  h->ms_lan = h->ms_vec = h->ms_xfer = h->ms_host_rule = h->ms_host_wall = 0.0;
  h->alpha.clear();
  h->beta.clear();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_set_weights(kmx_cert* h, const double* weight) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_cert_set_weights before kmx_cert_set_graph");
  std::string err;
  if (kmx::cert_check_weights(h->g.m, weight, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_cert_set_weights: " + err);
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  h->n_esc = 0;  // the candidates' costs were the old weights'
  if (int rc = ct_upload_weights(h, h->dev, h->g, weight)) return rc;
  if (h->have_point) {  // D - Lambda and the point's cost follow the weights
    if (int rc = ct_run_point(h)) return rc;
    KMX_HIP(hipMemcpyAsync(&h->cost, h->dev.scal.get(), sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KMX_HIP(hipStreamSynchronize(h->stream));
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_set_point(kmx_cert* h, int32_t r, const double* X, kmx_cert_point_info* info_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->have_graph, KMX_ESTATE, "kmx_cert_set_point before kmx_cert_set_graph");
  KMX_CHECK(r >= 3 && r <= 8, KMX_EINVAL, "kmx_cert_set_point: r must be in 3..8");
  KMX_CHECK(X, KMX_EINVAL, "null X");
  const size_t cnt = (size_t)h->g.n * (size_t)r * 4;
  for (size_t k = 0; k < cnt; ++k) KMX_CHECK(std::isfinite(X[k]), KMX_EINVAL, "kmx_cert_set_point: X not finite");
  KMX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  CtDev& d = h->dev;
  const int r_before = h->r;
  KMX_HIP(hipMemcpyAsync(d.X.get(), X, cnt * sizeof(double), hipMemcpyHostToDevice, s));
  h->r = r;
  h->have_point = false;  // the device's copy is being replaced
  h->n_esc = 0;
  KMX_HIP(hipEventRecord(h->ev[EV_POINT0], s));
  if (int rc = ct_run_point(h)) {
    h->r = r_before;
    return rc;
  }
  KMX_HIP(hipEventRecord(h->ev[EV_POINT1], s));
  double sc[3] = {0.0, 0.0, 0.0};
  KMX_HIP(hipMemcpyAsync(sc, d.scal.get(), sizeof(sc), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipStreamSynchronize(s));
  h->have_point = true;
  h->timed_point = true;
  h->cost = sc[0];
  if (info_out) {
    info_out->cost = sc[0];
    info_out->trace_lambda = sc[1];
    info_out->stationarity = std::sqrt(sc[2]);
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_escape(kmx_cert* h, const double* y, int32_t n_alpha, const double* alpha, double* cost_out,
                               int32_t* best_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && cost_out && best_out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->have_point, KMX_ESTATE, "kmx_cert_escape before kmx_cert_set_point");
  const kmx::CertGraph& g = h->g;
  const size_t N = (size_t)4 * g.n;
  std::string err;
  if (kmx::cert_escape_check(n_alpha, alpha, N, y, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_cert_escape: " + err);
  KMX_CHECK(h->r < 8, KMX_EUNSUP, "kmx_cert_escape: the point has rank 8 and there is no rank 9");
  CtDev& d = h->dev;
  const int r = h->r;
  KMX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  KMX_HIP(hipStreamSynchronize(s));
  const size_t need = (size_t)n_alpha * g.n * (size_t)(r + 1) * 4;
  if (d.cand.cap() < need) {  // the last escape's candidates go with the buffer, which goes before its successor comes
    h->n_esc = 0;
    d.cand.reset();
    if (int rc = d.cand.alloc(need)) return rc;
  }
  h->n_esc = 0;  // the buffer is being overwritten
  h->ms_esc = h->ms_esc_xfer = 0.0;
  double* d_alpha = d.esc.get();
  double* d_cost = d.esc.get() + kmx::CT_MAX_ALPHA;
  KMX_HIP(hipEventRecord(h->ev[EV_A], s));
  KMX_HIP(hipMemcpyAsync(d.y.get(), y, N * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipMemcpyAsync(d_alpha, alpha, (size_t)n_alpha * sizeof(double), hipMemcpyHostToDevice, s));
  KMX_HIP(hipEventRecord(h->ev[EV_B], s));
  const dim3 grid(g.n_tiles, n_alpha), wave(CT_TILE);
#define KMX_CT_ESCAPE(RR)                                                                                  \
  case RR:                                                                                                 \
    hipLaunchKernelGGL((k_ct_lift<RR>), grid, wave, 0, s, g.n, d.X.get(), d.y.get(), d_alpha, d.cand.get());\
    hipLaunchKernelGGL((k_ct_cost<RR + 1>), grid, wave, 0, s, g.n, d.ptr.get(), d.rec.get(), d.cand.get(), \
                       d.epart.get());                                                                     \
    break;
  switch (r) {
    KMX_CT_ESCAPE(3)
    KMX_CT_ESCAPE(4)
    KMX_CT_ESCAPE(5)
    KMX_CT_ESCAPE(6)
    KMX_CT_ESCAPE(7)
    default:
      return kmx::fail(KMX_EINVAL, "r outside 3..7");
  }
#undef KMX_CT_ESCAPE
  hipLaunchKernelGGL(k_ct_reduce, dim3(1), dim3(64), 0, s, g.n_tiles, n_alpha, d.epart.get(), d_cost, 0);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipEventRecord(h->ev[EV_C], s));
  double cost[kmx::CT_MAX_ALPHA];
  KMX_HIP(hipMemcpyAsync(cost, d_cost, (size_t)n_alpha * sizeof(double), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipEventRecord(h->ev[EV_D], s));
  KMX_HIP(hipStreamSynchronize(s));
  if (int rc = ct_span(h, EV_A, EV_B, &h->ms_esc_xfer)) return rc;
  if (int rc = ct_span(h, EV_B, EV_C, &h->ms_esc)) return rc;
  if (int rc = ct_span(h, EV_C, EV_D, &h->ms_esc_xfer)) return rc;
  for (int32_t k = 0; k < n_alpha; ++k) cost_out[k] = cost[k];
  *best_out = kmx::cert_escape_choose(n_alpha, cost, h->cost);
  h->n_esc = n_alpha;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_escape_commit(kmx_cert* h, int32_t k, double* X_out, kmx_cert_point_info* info_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && X_out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->have_point && h->n_esc > 0, KMX_ESTATE,
            "kmx_cert_escape_commit without the candidates of a kmx_cert_escape for this point and these weights");
  KMX_CHECK(k >= 0 && k < h->n_esc, KMX_EINVAL, "kmx_cert_escape_commit: k outside the last escape's candidates");
  CtDev& d = h->dev;
  const int r1 = h->r + 1;
  const size_t cnt = (size_t)h->g.n * (size_t)r1 * 4;
  KMX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const double* src = d.cand.get() + (size_t)k * cnt;
  KMX_HIP(hipMemcpyAsync(X_out, src, cnt * sizeof(double), hipMemcpyDeviceToHost, s));
  h->have_point = false;  // the device's copy is being replaced
  h->n_esc = 0;
  KMX_HIP(hipMemcpyAsync(d.X.get(), src, cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
  h->r = r1;
  KMX_HIP(hipEventRecord(h->ev[EV_POINT0], s));
  if (int rc = ct_run_point(h)) return rc;
  KMX_HIP(hipEventRecord(h->ev[EV_POINT1], s));
  double sc[3] = {0.0, 0.0, 0.0};
  KMX_HIP(hipMemcpyAsync(sc, d.scal.get(), sizeof(sc), hipMemcpyDeviceToHost, s));
  KMX_HIP(hipStreamSynchronize(s));
  h->have_point = true;
  h->timed_point = true;
  h->cost = sc[0];
  if (info_out) {
    info_out->cost = sc[0];
    info_out->trace_lambda = sc[1];
    info_out->stationarity = std::sqrt(sc[2]);
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_get_escape_timing(kmx_cert* h, double* ms) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && ms, KMX_EINVAL, "null argument");
  ms[0] = h->ms_esc;
  ms[1] = h->ms_esc_xfer;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_get_lambda(kmx_cert* h, double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->have_point, KMX_ESTATE, "kmx_cert_get_lambda before kmx_cert_set_point");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(out, h->dev.Lam.get(), (size_t)9 * h->g.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_apply(kmx_cert* h, const double* v_in, double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && v_in && out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->have_point, KMX_ESTATE, "kmx_cert_apply before kmx_cert_set_point");
  const kmx::CertGraph& g = h->g;
  CtDev& d = h->dev;
  const size_t bytes = (size_t)4 * g.n * sizeof(double);
  KMX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  KMX_HIP(hipMemcpyAsync(d.vec[0].get(), v_in, bytes, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_ct_apply, dim3(g.n_tiles), dim3(CT_TILE), 0, s, g.n, d.ptr.get(), d.rec.get(), d.Dm.get(),
                     d.vec[0].get(), nullptr, nullptr, 0, d.vec[1].get(), nullptr);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipMemcpyAsync(out, d.vec[1].get(), bytes, hipMemcpyDeviceToHost, s));
  KMX_HIP(hipStreamSynchronize(s));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_min_eig(kmx_cert* h, const kmx_cert_params* p, kmx_cert_result* res, double* y_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && res, KMX_EINVAL, "null argument");
  KMX_CHECK(h->have_point, KMX_ESTATE, "kmx_cert_min_eig before kmx_cert_set_point");
  kmx::CertParams P;
  std::string err;
  if (kmx::cert_params(p, &P, &err) != KMX_OK) return kmx::fail(KMX_EINVAL, "kmx_cert_min_eig: " + err);
  const kmx::CertGraph& g = h->g;
  CtDev& d = h->dev;
  const size_t N = (size_t)4 * g.n;
  KMX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  KMX_HIP(hipStreamSynchronize(s));
  if (d.sv.cap() < (size_t)P.max_steps + 1) {
    d.alpha.reset();
    d.B.reset();
    d.sv.reset();
    int rc = KMX_OK;
    if ((rc = d.alpha.alloc((size_t)P.max_steps + 1)) || (rc = d.B.alloc((size_t)P.max_steps + 1)) ||
        (rc = d.sv.alloc((size_t)P.max_steps + 1)))
      return rc;
  }
  std::vector<double> u0(N);
  kmx::cert_start_vector(P.seed, N, u0.data());
  std::vector<double> alpha((size_t)P.max_steps), B((size_t)P.max_steps + 1);
  h->alpha.clear();
  h->beta.clear();
  h->ms_lan = h->ms_vec = h->ms_xfer = h->ms_host_rule = h->ms_host_wall = 0.0;
  const double t_call = ct_now_ms();
  const size_t vbytes = N * sizeof(double);
  KMX_HIP(hipEventRecord(h->ev[EV_A], s));
  KMX_HIP(hipMemcpyAsync(d.vec[0].get(), u0.data(), vbytes, hipMemcpyHostToDevice, s));
  KMX_HIP(hipEventRecord(h->ev[EV_B], s));
  if (int rc = ct_start_norm(h)) return rc;
  kmx::CertScan scan;
  int done = 0;
  while (done < P.max_steps && !scan.done) {
    // a batch: EV_B .. EV_C the steps (the first batch's with the start vector's norm), EV_C .. EV_D the read-back
    const int k = std::min(P.check_every, P.max_steps - done);
    if (done > 0) KMX_HIP(hipEventRecord(h->ev[EV_B], s));
    ct_enqueue_steps<false>(h, done, k);
    KMX_HIP(hipGetLastError());
    KMX_HIP(hipEventRecord(h->ev[EV_C], s));
    KMX_HIP(hipMemcpyAsync(alpha.data() + done, d.alpha.get() + done, (size_t)k * sizeof(double), hipMemcpyDeviceToHost,
                           s));
    KMX_HIP(hipMemcpyAsync(B.data() + done + 1, d.B.get() + done + 1, (size_t)k * sizeof(double), hipMemcpyDeviceToHost,
                           s));
    KMX_HIP(hipEventRecord(h->ev[EV_D], s));
    KMX_HIP(hipStreamSynchronize(s));
    if (done == 0)
      if (int rc = ct_span(h, EV_A, EV_B, &h->ms_xfer)) return rc;
    if (int rc = ct_span(h, EV_B, EV_C, &h->ms_lan)) return rc;
    if (int rc = ct_span(h, EV_C, EV_D, &h->ms_xfer)) return rc;
    const double t_rule = ct_now_ms();
    for (int j = done + 1; j <= done + k && !scan.done; ++j) {
      if (kmx::cert_scan_step(&scan, j, alpha.data(), B.data() + 1, P, &err) != KMX_OK)
        return kmx::fail(KMX_EINVAL, "kmx_cert_min_eig: " + err);
      h->alpha.push_back(alpha[(size_t)j - 1]);
      h->beta.push_back(B[(size_t)j]);
    }
    h->ms_host_rule += ct_now_ms() - t_rule;
    done += k;
  }
  *res = scan.res;
  if (y_out) {
    // the second pass: the same steps from the same start, y = sum_j s_j v_j
    const int ks = scan.res.steps;
    KMX_HIP(hipEventRecord(h->ev[EV_A], s));
    KMX_HIP(hipMemcpyAsync(d.sv.get(), scan.s.data(), (size_t)ks * sizeof(double), hipMemcpyHostToDevice, s));
    KMX_HIP(hipMemcpyAsync(d.vec[0].get(), u0.data(), vbytes, hipMemcpyHostToDevice, s));
    KMX_HIP(hipEventRecord(h->ev[EV_B], s));
    KMX_HIP(hipMemsetAsync(d.y.get(), 0, vbytes, s));
    if (int rc = ct_start_norm(h)) return rc;
    ct_enqueue_steps<true>(h, 0, ks);
    KMX_HIP(hipGetLastError());
    KMX_HIP(hipEventRecord(h->ev[EV_C], s));
    KMX_HIP(hipMemcpyAsync(y_out, d.y.get(), vbytes, hipMemcpyDeviceToHost, s));
    KMX_HIP(hipEventRecord(h->ev[EV_D], s));
    KMX_HIP(hipStreamSynchronize(s));
    if (int rc = ct_span(h, EV_A, EV_B, &h->ms_xfer)) return rc;
    if (int rc = ct_span(h, EV_B, EV_C, &h->ms_vec)) return rc;
    if (int rc = ct_span(h, EV_C, EV_D, &h->ms_xfer)) return rc;
    double nn = 0.0;  // in index order
    for (size_t k = 0; k < N; ++k) nn += y_out[k] * y_out[k];
    nn = std::sqrt(nn);
    if (nn > 0 && std::isfinite(nn))
      for (size_t k = 0; k < N; ++k) y_out[k] /= nn;
  }
  h->ms_host_wall = ct_now_ms() - t_call;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_get_coefficients(kmx_cert* h, int32_t capacity, double* alpha_out, double* beta_out,
                                         int32_t* count_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && count_out, KMX_EINVAL, "null argument");
  KMX_CHECK(capacity >= 0 && (capacity == 0 || (alpha_out && beta_out)), KMX_EINVAL, "bad capacity / null output");
  const int32_t cnt = (int32_t)h->alpha.size();
  *count_out = cnt;
  for (int32_t k = 0; k < std::min(cnt, capacity); ++k) {
    alpha_out[k] = h->alpha[(size_t)k];
    beta_out[k] = h->beta[(size_t)k];
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_ritz(int32_t k, const double* alpha, const double* beta, double eta, kmx_cert_result* res) {
  KMX_GUARD_BEGIN
  std::string err;
  if (kmx::cert_ritz(k, alpha, beta, eta, res, nullptr, &err) != KMX_OK)
    return kmx::fail(KMX_EINVAL, "kmx_cert_ritz: " + err);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_start_vector(uint64_t seed, int64_t count, double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(count >= 0 && (count == 0 || out), KMX_EINVAL, "bad count / null output");
  kmx::cert_start_vector(seed, (size_t)count, out);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_get_timing(kmx_cert* h, double* ms) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && ms, KMX_EINVAL, "null argument");
  KMX_CHECK(h->timed_point, KMX_ESTATE, "kmx_cert_get_timing before kmx_cert_set_point");
  KMX_HIP(hipSetDevice(h->device));
  ms[0] = 0.0;
  if (int rc = ct_span(h, EV_POINT0, EV_POINT1, &ms[0])) return rc;
  ms[1] = h->ms_lan;
  ms[2] = h->ms_vec;
  ms[3] = h->ms_xfer;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_cert_get_host_timing(kmx_cert* h, double* ms) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && ms, KMX_EINVAL, "null argument");
  ms[0] = h->ms_host_rule;
  ms[1] = h->ms_host_wall;
  return KMX_OK;
  KMX_GUARD_END
}
