// cert_host.h — host-side half of cert.hip that needs no device: the checks
// kmx_cert_set_graph / kmx_cert_set_weights run before any device call, the
// per-pose incidence CSR they upload, the start vector of the Lanczos
// iteration, and the tridiagonal eigensolver with the decision rule
// (kmx_cert_ritz), and the argument checks and the choice rule of
// kmx_cert_escape. Plain C++, so `make cert_check` and `make stair_check` can
// build it with the host sanitizers (cert_check.cpp, stair_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "graph_host.h"
#include "kmx_abi.h"

namespace kmx {

constexpr int CT_TILE = 64;               // poses per tile = lanes per workgroup (one wave)
constexpr uint32_t CT_TAIL = GRAPH_TAIL;  // record bit: this pose is the edge's tail (p == i): it applies C
// CERTIFIED needs rho <= CT_RESIDUAL_FACTOR * eta. Lanczos converges to the kernel of S (the rows of X)
// before it resolves a negative eigenvalue just below it, and with rho up to eta that gave false
// certificates at lambda_min between -eta and -3 eta: 20 of 1350 runs on almost stationary points.
// The largest of 1, 1/2, 1/4, 1/10, 1/100 with none there (tests/test_cert_sound_cpu.py).
constexpr double CT_RESIDUAL_FACTOR = 0.1;

// What kmx_cert_set_graph keeps: the incidence CSR of the team graph (sorted
// by pose, in edge order within a pose). There are no blocks: S couples robots.
struct CertGraph {
  int32_t n = 0;
  int64_t m = 0;
  std::vector<int32_t> inc_ptr;     // [n + 1]
  std::vector<uint32_t> inc_other;  // [2m] other endpoint | CT_TAIL
  std::vector<int32_t> inc_edge;    // [2m] the caller's edge index (weights are per edge)
  std::vector<double> kappa, tau;   // [m]
  int32_t n_tiles = 0;
};

// weight NULL: 1. KMX_OK, or KMX_EINVAL with *err set.
inline int cert_check_weights(int64_t m, const double* weight, std::string* err) {
  if (weight)
    for (int64_t e = 0; e < m; ++e)
      if (!std::isfinite(weight[e]) || weight[e] < 0) {
        if (err) *err = "weight must be finite and >= 0 (edge " + std::to_string(e) + ")";
        return KMX_EINVAL;
      }
  return KMX_OK;
}

// Checks the arguments of kmx_cert_set_graph and, when they pass, builds *out
// (untouched on failure). KMX_OK, or KMX_EINVAL with *err set.
inline int cert_build(int32_t n, int64_t m, const int32_t* src, const int32_t* dst, const double* R, const double* t,
                      const double* kappa, const double* tau, const double* weight, CertGraph* out,
                      std::string* err) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  if (!out) return bad("null argument");
  if (n < 1 || m < 0) return bad("bad argument (n_poses >= 1, n_edges >= 0)");
  if (m > 0 && (!src || !dst || !R || !t || !kappa || !tau)) return bad("null edge array");
  if (m >= (int64_t)INT32_MAX / 2) return bad("too many edges (2 * n_edges must fit int32)");
  if (n >= INT32_MAX / 8) return bad("too many poses");
  std::string werr = graph_check_edges(n, m, src, dst, R, t, kappa, tau, [](int64_t) { return (const char*)nullptr; });
  if (!werr.empty()) return bad(werr);
  if (cert_check_weights(m, weight, &werr) != KMX_OK) return bad(werr);

  CertGraph g;
  g.n = n;
  g.m = m;
  g.kappa.assign(kappa, kappa + m);
  g.tau.assign(tau, tau + m);
  graph_incidence_csr(n, m, src, dst, &g.inc_ptr, &g.inc_other, &g.inc_edge);
  g.n_tiles = (n + CT_TILE - 1) / CT_TILE;
  *out = std::move(g);
  return KMX_OK;
}

// The per-record weights w*kappa and w*tau the kernels read, interleaved
// [rec][2] (weight NULL: 1).
inline void cert_record_weights(const CertGraph& g, const double* weight, std::vector<double>* wkt) {
  const size_t nrec = g.inc_edge.size();
  wkt->resize(2 * nrec);
  for (size_t k = 0; k < nrec; ++k) {
    const int32_t e = g.inc_edge[k];
    const double w = weight ? weight[e] : 1.0;
    (*wkt)[2 * k] = w * g.kappa[e];
    (*wkt)[2 * k + 1] = w * g.tau[e];
  }
}

// The start vector before its normalisation: splitmix64 of seed and the index,
// 53 bits to [-1, 1). Every value is exact, so any restatement gives its bits.
inline void cert_start_vector(uint64_t seed, size_t count, double* out) {
  for (size_t i = 0; i < count; ++i) {
    uint64_t z = seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    out[i] = (double)(z >> 11) * 0x1p-52 - 1.0;
  }
}

// kmx_cert_params with the defaults filled in.
struct CertParams {
  double eta = 0.0;
  int32_t max_steps = 5000, test_every = 10, check_every = 50;
  uint64_t seed = 0;
};

inline int cert_params(const kmx_cert_params* p, CertParams* out, std::string* err) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  if (!p) return bad("null params (eta is required)");
  if (!std::isfinite(p->eta) || !(p->eta > 0)) return bad("eta must be finite and > 0");
  if (p->max_steps < 0 || p->test_every < 0 || p->check_every < 0)
    return bad("max_steps, test_every and check_every must be >= 0 (0: the default)");
  if (p->reserved != 0) return bad("reserved must be 0");
  CertParams c;
  c.eta = p->eta;
  if (p->max_steps > 0) c.max_steps = p->max_steps;
  if (p->test_every > 0) c.test_every = p->test_every;
  if (p->check_every > 0) c.check_every = p->check_every;
  c.seed = p->seed;
  if (out) *out = c;
  return KMX_OK;
}

namespace cert_detail {

constexpr int MS = 7;  // shifts per pass of the Sturm count: independent chains, so their divisions overlap

// Eigenvalues of the k x k tridiagonal (a, b[0..k-2]) below each of the MS shifts x.
inline void sturm_counts(int k, const double* a, const double* b, const double* x, double pivmin, int* cnt) {
  double q[MS];
  for (int s = 0; s < MS; ++s) {
    q[s] = a[0] - x[s];
    if (std::fabs(q[s]) < pivmin) q[s] = -pivmin;
    cnt[s] = q[s] < 0;
  }
  for (int i = 1; i < k; ++i) {
    const double bb = b[i - 1] * b[i - 1], ai = a[i];
    for (int s = 0; s < MS; ++s) {
      double v = (ai - x[s]) - bb / q[s];
      if (std::fabs(v) < pivmin) v = -pivmin;
      cnt[s] += v < 0;
      q[s] = v;
    }
  }
}

struct TriBounds {
  double lo, hi;   // Gershgorin, padded
  double tnorm;    // a bound of |T|
  double pivmin;   // the smallest pivot of the Sturm count
  double tol;      // where the bisection stops: the accuracy the count itself has
  double pad;      // what a computed eigenvalue may be off by
};

inline TriBounds tri_bounds(int k, const double* alpha, const double* beta) {
  TriBounds B;
  B.lo = B.hi = alpha[0];
  B.tnorm = 0.0;
  for (int i = 0; i < k; ++i) {
    const double r = (i > 0 ? std::fabs(beta[i - 1]) : 0.0) + (i + 1 < k ? std::fabs(beta[i]) : 0.0);
    B.lo = std::min(B.lo, alpha[i] - r);
    B.hi = std::max(B.hi, alpha[i] + r);
    B.tnorm = std::max(B.tnorm, std::fabs(alpha[i]) + r);
  }
  const double eps = std::numeric_limits<double>::epsilon();
  B.pivmin = std::max(std::numeric_limits<double>::min(), eps * eps * B.tnorm);
  B.tol = eps * B.tnorm;
  B.pad = 2.0 * eps * B.tnorm * k + 2.0 * B.pivmin;
  B.lo -= B.pad;
  B.hi += B.pad;
  return B;
}

// The eigenvalue of index idx (0: smallest) inside [lo, hi] (count(lo) <= idx <
// count(hi)): MS + 1 sections per pass until the interval is below tol.
inline double multisect(int k, const double* a, const double* b, int idx, double lo, double hi, const TriBounds& B) {
  for (int it = 0; it < 400 && hi - lo > B.tol; ++it) {
    double x[MS];
    int cnt[MS];
    const double h = (hi - lo) / (MS + 1);
    for (int s = 0; s < MS; ++s) x[s] = lo + h * (s + 1);
    if (!(x[0] > lo) || !(x[MS - 1] < hi)) break;  // the interval holds no more doubles to tell apart
    sturm_counts(k, a, b, x, B.pivmin, cnt);
    int s = 0;
    while (s < MS && cnt[s] <= idx) ++s;  // the first shift above the eigenvalue
    if (s > 0) lo = x[s - 1];
    if (s < MS) hi = x[s];
  }
  return lo + 0.5 * (hi - lo);
}

// The smallest eigenvalue. upper (or NULL): a value it cannot exceed, the
// smallest eigenvalue of a leading block (Cauchy interlacing: the smallest Ritz
// value does not grow with the step count). One pass of shifts spaced
// geometrically below it finds the bracket; close to convergence that bracket
// is a few tol wide and the search ends in a pass or two.
inline double theta_min(int k, const double* a, const double* b, const TriBounds& B, const double* upper) {
  if (k == 1) return a[0];
  double lo = B.lo, hi = B.hi;
  if (upper && *upper + B.pad < hi) {
    const double top = *upper + B.pad, g = std::max(B.pad, B.tol);
    double x[MS], f = 1.0;
    int cnt[MS];
    x[0] = top;
    for (int s = 1; s < MS; ++s) {
      f *= 16.0;
      x[s] = std::max(top - g * f, B.lo);
    }
    sturm_counts(k, a, b, x, B.pivmin, cnt);
    if (cnt[0] > 0) {  // otherwise the bound did not hold: the full bracket
      int s = 0;
      while (s + 1 < MS && cnt[s + 1] > 0) ++s;  // the lowest shift still above the eigenvalue
      hi = x[s];
      lo = s + 1 < MS ? x[s + 1] : B.lo;
    }
  }
  return multisect(k, a, b, 0, lo, hi, B);
}

inline double theta_max(int k, const double* a, const double* b, const TriBounds& B) {
  return k == 1 ? a[0] : multisect(k, a, b, k - 1, B.lo, B.hi, B);
}

// The unit eigenvector x [k] of the eigenvalue theta: inverse iteration with a
// partially pivoted LU of T - theta I (zero pivots replaced by eps |T|) from a
// fixed start.
inline void eigvec(int k, const double* alpha, const double* beta, double theta, const TriBounds& B,
                   std::vector<double>* s_out) {
  std::vector<double>& x = *s_out;
  x.assign((size_t)k, 1.0);
  if (k == 1) return;
  // U has three diagonals (rows i, i + 1 may swap)
  std::vector<double> d((size_t)k), du((size_t)k, 0.0), du2((size_t)k, 0.0), l((size_t)k, 0.0);
  std::vector<uint8_t> swp((size_t)k, 0);
  const double tiny = std::max(B.tol, std::numeric_limits<double>::min());
  for (int i = 0; i < k; ++i) d[i] = alpha[i] - theta;
  for (int i = 0; i + 1 < k; ++i) du[i] = beta[i];
  for (int i = 0; i + 1 < k; ++i) {
    const double sub = beta[i];
    if (std::fabs(d[i]) >= std::fabs(sub)) {
      if (d[i] == 0.0) d[i] = tiny;
      l[i] = sub / d[i];
      d[i + 1] -= l[i] * du[i];
    } else {  // swap rows i and i + 1
      swp[i] = 1;
      l[i] = d[i] / sub;
      const double di = d[i + 1], dui = du[i];
      d[i] = sub;
      du[i] = di;
      d[i + 1] = dui - l[i] * di;
      if (i + 2 < k) {
        du2[i] = du[i + 1];
        du[i + 1] = -l[i] * du2[i];
      }
    }
  }
  for (int i = 0; i < k; ++i)
    if (std::fabs(d[i]) < tiny) d[i] = d[i] < 0 ? -tiny : tiny;
  // a fixed start without a pattern (splitmix64 of the index)
  cert_start_vector(0x5EEDull, (size_t)k, x.data());
  for (int it = 0; it < 4; ++it) {
    double nn = 0.0;
    for (int i = 0; i < k; ++i) nn = std::max(nn, std::fabs(x[i]));
    if (!(nn > 0) || !std::isfinite(nn)) break;
    for (int i = 0; i < k; ++i) x[i] /= nn;
    for (int i = 0; i + 1 < k; ++i) {  // forward: L^-1 P x
      if (swp[i]) std::swap(x[i], x[i + 1]);
      x[i + 1] -= l[i] * x[i];
    }
    for (int i = k - 1; i >= 0; --i) {  // back: U^-1
      double v = x[i];
      if (i + 1 < k) v -= du[i] * x[i + 1];
      if (i + 2 < k) v -= du2[i] * x[i + 2];
      x[i] = v / d[i];
    }
  }
  double nn = 0.0, mx = 0.0;
  for (int i = 0; i < k; ++i) mx = std::max(mx, std::fabs(x[i]));
  if (mx > 0 && std::isfinite(mx)) {
    for (int i = 0; i < k; ++i) {
      x[i] /= mx;
      nn += x[i] * x[i];
    }
    nn = std::sqrt(nn);
    for (int i = 0; i < k; ++i) x[i] /= nn;
  } else {
    x.assign((size_t)k, 0.0);
    x[0] = 1.0;
  }
}

}  // namespace cert_detail

// The decision rule on the first k Lanczos steps (alpha[0..k-1], beta[0..k-1];
// beta[k-1] is the norm left after step k). theta_min is the smallest Ritz
// value and rho = |beta[k-1] s_k| its residual bound (s: its unit eigenvector
// in the tridiagonal):
//   NEGATIVE  if theta_min < -eta (Ritz values lie inside the spectrum);
//   CERTIFIED if rho <= CT_RESIDUAL_FACTOR * eta and theta_min - rho >= -eta;
//   UNDECIDED otherwise (the caller goes on).
// CERTIFIED is a residual statement: S has an eigenvalue within rho of theta_min, and theta_min is the
// smallest one this Krylov space shows. No Lanczos rule bounds lambda_min from below; the factor asks
// for a resolution an order finer than the threshold before the space is believed.
// The eigenvalues come from multisection on the Sturm count, to eps |T|.
// s_out (or NULL): the Ritz vector's coordinates [k]. upper (or NULL): a bound
// theta_min cannot exceed (the theta_min of fewer steps). lazy_max: theta_max
// is not needed when the outcome is UNDECIDED (it is then reported as NaN).
inline int cert_ritz(int k, const double* alpha, const double* beta, double eta, kmx_cert_result* res,
                     std::vector<double>* s_out, std::string* err, const double* upper = nullptr,
                     bool lazy_max = false) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  if (k < 1 || !alpha || !beta || !res) return bad("bad argument (k >= 1, arrays not null)");
  if (!std::isfinite(eta) || !(eta > 0)) return bad("eta must be finite and > 0");
  for (int i = 0; i < k; ++i)
    if (!std::isfinite(alpha[i]) || !std::isfinite(beta[i])) return bad("alpha / beta not finite");
  const cert_detail::TriBounds B = cert_detail::tri_bounds(k, alpha, beta);
  const double tmin = cert_detail::theta_min(k, alpha, beta, B, upper);
  std::vector<double> s;
  cert_detail::eigvec(k, alpha, beta, tmin, B, &s);
  const double rho = std::fabs(beta[k - 1] * s[(size_t)k - 1]);
  res->steps = k;
  res->theta_min = tmin;
  res->residual = rho;
  if (tmin < -eta)
    res->decision = KMX_CERT_NEGATIVE;
  else if (rho <= CT_RESIDUAL_FACTOR * eta && tmin - rho >= -eta)
    res->decision = KMX_CERT_CERTIFIED;
  else
    res->decision = KMX_CERT_UNDECIDED;
  res->theta_max = lazy_max && res->decision == KMX_CERT_UNDECIDED ? std::numeric_limits<double>::quiet_NaN()
                                                                    : cert_detail::theta_max(k, alpha, beta, B);
  if (s_out) *s_out = std::move(s);
  return KMX_OK;
}

// What the host does with the coefficients as they arrive: steps are taken in
// order, whatever the batch they came in, so the outcome does not depend on
// check_every. A breakdown (beta at the rounding level of the tridiagonal's
// norm: the Krylov space is invariant) ends the iteration with the rule applied
// to that prefix; otherwise the rule is applied at multiples of test_every.
// Each test brackets theta_min from the one before, so a test costs a few
// passes over the k coefficients and not a full bisection.
struct CertScan {
  double scale = 0.0;  // running bound of |T|
  bool done = false, breakdown = false;
  bool have_upper = false;
  double upper = 0.0;  // theta_min of the last test
  kmx_cert_result res{};
  std::vector<double> s;
};

inline int cert_scan_step(CertScan* sc, int j /* step count, 1-based */, const double* alpha, const double* beta,
                          const CertParams& p, std::string* err) {
  const double a = alpha[j - 1], b = beta[j - 1];
  if (!std::isfinite(a) || !std::isfinite(b)) {
    if (err) *err = "a Lanczos coefficient is not finite (step " + std::to_string(j) + ")";
    return KMX_EINVAL;
  }
  sc->scale = std::max(sc->scale, std::fabs(a) + b + (j > 1 ? beta[j - 2] : 0.0));
  const bool brk = b <= 1e-14 * sc->scale;
  const bool last = j == p.max_steps;
  if (!brk && !last && j % p.test_every != 0) return KMX_OK;
  if (int rc = cert_ritz(j, alpha, beta, p.eta, &sc->res, &sc->s, err, sc->have_upper ? &sc->upper : nullptr,
                         !brk && !last))
    return rc;
  sc->upper = sc->res.theta_min;
  sc->have_upper = true;
  if (brk) {
    sc->breakdown = sc->done = true;
  } else if (j % p.test_every != 0) {  // the last step, not a test step: reported, not decided
    sc->res.decision = KMX_CERT_UNDECIDED;
    sc->done = true;
  } else if (sc->res.decision != KMX_CERT_UNDECIDED || last) {
    sc->done = true;
  }
  return KMX_OK;
}

// ---- the escape step of the Riemannian staircase (kmx_cert_escape)

constexpr int32_t CT_MAX_ALPHA = 8;  // candidates per kmx_cert_escape call

// The arguments of kmx_cert_escape: 1..CT_MAX_ALPHA step lengths, all finite,
// and a finite direction y [ny]. KMX_OK, or KMX_EINVAL with *err set.
inline int cert_escape_check(int32_t n_alpha, const double* alpha, size_t ny, const double* y, std::string* err) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  if (n_alpha < 1 || n_alpha > CT_MAX_ALPHA)
    return bad("n_alpha must be in 1.." + std::to_string(CT_MAX_ALPHA) + ", got " + std::to_string(n_alpha));
  if (!alpha || !y) return bad("null argument");
  for (int32_t k = 0; k < n_alpha; ++k)
    if (!std::isfinite(alpha[k])) return bad("alpha not finite (index " + std::to_string(k) + ")");
  for (size_t i = 0; i < ny; ++i)
    if (!std::isfinite(y[i])) return bad("y not finite (index " + std::to_string(i) + ")");
  return KMX_OK;
}

// The candidate kmx_cert_escape reports: the lowest finite cost strictly below
// the point's own cost0, ties to the earlier index; -1 when no candidate
// descends (a cost that is not finite is never chosen, and neither is any
// candidate when cost0 is not finite).
inline int32_t cert_escape_choose(int32_t n_alpha, const double* cost, double cost0) {
  int32_t best = -1;
  if (!cost || !std::isfinite(cost0)) return best;
  for (int32_t k = 0; k < n_alpha; ++k) {
    if (!std::isfinite(cost[k]) || !(cost[k] < cost0)) continue;
    if (best < 0 || cost[k] < cost[best]) best = k;
  }
  return best;
}

}  // namespace kmx
