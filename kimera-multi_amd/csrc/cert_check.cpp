// cert_check.cpp — cert.hip's host code (cert_host.h: the checks of
// kmx_cert_set_graph / kmx_cert_set_weights and the incidence CSR they build,
// the start vector, the tridiagonal eigensolver and the decision rule of
// kmx_cert_min_eig / kmx_cert_ritz) as a stand-alone program, built by
// `make cert_check` with the host address and undefined-behaviour sanitizers.
// Every array is passed in a vector of exactly the stated size, so a read past
// one is a report. CPU only.
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "cert_host.h"

namespace {

int g_fail = 0;

struct Graph {
  int32_t n = 0;
  std::vector<int32_t> src, dst;
  std::vector<double> R, t, kappa, tau, weight;
  bool with_weight = true;

  void edge(int32_t i, int32_t j, double k = 2.0, double ta = 3.0, double w = 1.0) {
    src.push_back(i);
    dst.push_back(j);
    const double c = std::cos(0.1 * (double)src.size()), s = std::sin(0.1 * (double)src.size());
    const double Re[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    R.insert(R.end(), Re, Re + 9);
    for (int q = 0; q < 3; ++q) t.push_back(0.5 * q + (double)src.size());
    kappa.push_back(k);
    tau.push_back(ta);
    weight.push_back(w);
  }
  int build(kmx::CertGraph* out, std::string* err) const {
    std::vector<int32_t> s(src), d(dst);  // exact-size copies
    std::vector<double> r(R), tt(t), k(kappa), ta(tau), w(weight);
    return kmx::cert_build(n, (int64_t)s.size(), s.empty() ? nullptr : s.data(), d.empty() ? nullptr : d.data(),
                           r.empty() ? nullptr : r.data(), tt.empty() ? nullptr : tt.data(),
                           k.empty() ? nullptr : k.data(), ta.empty() ? nullptr : ta.data(),
                           with_weight && !w.empty() ? w.data() : nullptr, out, err);
  }
};

void expect(const Graph& g, int code, const char* what, const char* name) {
  kmx::CertGraph out;
  out.n = -7;  // a failed build must leave *out alone
  std::string err;
  const int rc = g.build(&out, &err);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos) || (code != KMX_OK && out.n != -7)) {
    std::fprintf(stderr, "%s: expected %d (%s), got %d (%s)\n", name, code, what, rc, err.c_str());
    ++g_fail;
  }
}

Graph chain(int32_t n) {
  Graph g;
  g.n = n;
  for (int32_t p = 0; p + 1 < n; ++p) g.edge(p, p + 1);
  return g;
}

// The CSR against the edge list: every edge appears once at each end, in edge
// order within a pose, with the tail flag at its source; the record weights
// follow the caller's.
void check_csr(const Graph& g, const char* name) {
  auto fail = [&](const char* m) {
    std::fprintf(stderr, "%s: CSR: %s\n", name, m);
    ++g_fail;
  };
  kmx::CertGraph c;
  std::string err;
  if (g.build(&c, &err) != KMX_OK) return fail(err.c_str());
  const size_t m = g.src.size();
  if (c.n != g.n || c.m != (int64_t)m || c.n_tiles != (g.n + kmx::CT_TILE - 1) / kmx::CT_TILE) return fail("sizes");
  if (c.inc_ptr.size() != (size_t)g.n + 1 || c.inc_ptr[0] != 0 || (size_t)c.inc_ptr[g.n] != 2 * m)
    return fail("inc_ptr");
  if (c.inc_other.size() != 2 * m || c.inc_edge.size() != 2 * m) return fail("record arrays");
  std::vector<int> seen_tail(m, 0), seen_head(m, 0);
  for (int32_t p = 0; p < g.n; ++p) {
    if (c.inc_ptr[p + 1] < c.inc_ptr[p]) return fail("inc_ptr not monotone");
    int32_t last = -1;
    for (int32_t k = c.inc_ptr[p]; k < c.inc_ptr[p + 1]; ++k) {
      const int32_t e = c.inc_edge[k];
      if (e < 0 || (size_t)e >= m) return fail("edge index");
      if (e <= last) return fail("records not in edge order");
      last = e;
      const bool tail = (c.inc_other[k] & kmx::CT_TAIL) != 0;
      const int32_t o = (int32_t)(c.inc_other[k] & 0x7fffffffu);
      if (tail ? (g.src[e] != p || g.dst[e] != o) : (g.dst[e] != p || g.src[e] != o)) return fail("endpoints");
      (tail ? seen_tail : seen_head)[e]++;
    }
  }
  for (size_t e = 0; e < m; ++e)
    if (seen_tail[e] != 1 || seen_head[e] != 1) return fail("an edge is not at both ends once");
  std::vector<double> wkt;
  std::vector<double> w(g.weight);
  kmx::cert_record_weights(c, g.with_weight && !w.empty() ? w.data() : nullptr, &wkt);
  if (wkt.size() != 4 * m) return fail("record weights size");
  for (size_t k = 0; k < 2 * m; ++k) {
    const int32_t e = c.inc_edge[k];
    const double ww = g.with_weight ? g.weight[e] : 1.0;
    if (wkt[2 * k] != ww * g.kappa[e] || wkt[2 * k + 1] != ww * g.tau[e]) return fail("record weights");
  }
}

// Jacobi eigenvalues of a small symmetric matrix (the reference for the
// tridiagonal solver): returns the sorted eigenvalues and the eigenvectors.
void jacobi(int k, std::vector<double> A, std::vector<double>* ev, std::vector<double>* V) {
  V->assign((size_t)k * k, 0.0);
  for (int i = 0; i < k; ++i) (*V)[(size_t)i * k + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < k; ++i)
      for (int j = i + 1; j < k; ++j) off += A[(size_t)i * k + j] * A[(size_t)i * k + j];
    if (off < 1e-300) break;
    for (int p = 0; p < k; ++p)
      for (int q = p + 1; q < k; ++q) {
        const double apq = A[(size_t)p * k + q];
        if (apq == 0.0) continue;
        const double th = (A[(size_t)q * k + q] - A[(size_t)p * k + p]) / (2.0 * apq);
        const double tt = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(1.0 + th * th));
        const double cs = 1.0 / std::sqrt(1.0 + tt * tt), sn = cs * tt;
        for (int r = 0; r < k; ++r) {
          const double arp = A[(size_t)r * k + p], arq = A[(size_t)r * k + q];
          A[(size_t)r * k + p] = cs * arp - sn * arq;
          A[(size_t)r * k + q] = sn * arp + cs * arq;
        }
        for (int r = 0; r < k; ++r) {
          const double apr = A[(size_t)p * k + r], aqr = A[(size_t)q * k + r];
          A[(size_t)p * k + r] = cs * apr - sn * aqr;
          A[(size_t)q * k + r] = sn * apr + cs * aqr;
        }
        for (int r = 0; r < k; ++r) {
          const double vp = (*V)[(size_t)r * k + p], vq = (*V)[(size_t)r * k + q];
          (*V)[(size_t)r * k + p] = cs * vp - sn * vq;
          (*V)[(size_t)r * k + q] = sn * vp + cs * vq;
        }
      }
  }
  ev->resize((size_t)k);
  for (int i = 0; i < k; ++i) (*ev)[i] = A[(size_t)i * k + i];
}

int check_tridiag(std::mt19937& rng, int k, double shift) {
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::vector<double> a((size_t)k), b((size_t)k);
  for (int i = 0; i < k; ++i) {
    a[i] = 3.0 * U(rng) + shift;
    b[i] = 0.1 + std::fabs(U(rng));
  }
  std::vector<double> A((size_t)k * k, 0.0), ev, V;
  for (int i = 0; i < k; ++i) {
    A[(size_t)i * k + i] = a[i];
    if (i + 1 < k) A[(size_t)i * k + i + 1] = A[(size_t)(i + 1) * k + i] = b[i];
  }
  jacobi(k, A, &ev, &V);
  int imin = 0, imax = 0;
  for (int i = 0; i < k; ++i) {
    if (ev[i] < ev[imin]) imin = i;
    if (ev[i] > ev[imax]) imax = i;
  }
  kmx_cert_result res;
  std::vector<double> s;
  std::string err;
  const double eta = 0.05;
  std::vector<double> ac(a), bc(b);  // exact-size copies
  if (kmx::cert_ritz(k, ac.data(), bc.data(), eta, &res, &s, &err) != KMX_OK) {
    std::fprintf(stderr, "cert_ritz refused a good tridiagonal: %s\n", err.c_str());
    return ++g_fail;
  }
  const double scale = std::max(std::fabs(ev[imin]), std::fabs(ev[imax])) + 1.0;
  const double rho = std::fabs(b[k - 1] * V[(size_t)(k - 1) * k + imin]);
  bool ok = std::fabs(res.theta_min - ev[imin]) <= 1e-12 * scale && std::fabs(res.theta_max - ev[imax]) <= 1e-12 * scale &&
            res.steps == k && (int)s.size() == k;
  // the eigenvector is compared only where the smallest eigenvalue is isolated
  double gap = std::numeric_limits<double>::infinity();
  for (int i = 0; i < k; ++i)
    if (i != imin) gap = std::min(gap, ev[i] - ev[imin]);
  if (gap > 1e-3) ok = ok && std::fabs(res.residual - rho) <= 1e-11 * scale / gap;
  const int want = res.theta_min < -eta ? KMX_CERT_NEGATIVE
                   : (res.residual <= kmx::CT_RESIDUAL_FACTOR * eta && res.theta_min - res.residual >= -eta)
                       ? KMX_CERT_CERTIFIED
                       : KMX_CERT_UNDECIDED;
  ok = ok && res.decision == want;
  if (!ok) {
    std::fprintf(stderr, "tridiagonal k=%d: theta %.17g / %.17g vs %.17g / %.17g, rho %.3e vs %.3e, decision %d\n", k,
                 res.theta_min, res.theta_max, ev[imin], ev[imax], res.residual, rho, res.decision);
    ++g_fail;
  }
  return res.decision;
}

}  // namespace

int main() {
  int refused = 0;
  auto bad = [&](Graph g, const char* what, const char* name) {
    expect(g, KMX_EINVAL, what, name);
    ++refused;
  };
  {
    Graph g = chain(5);
    g.src[2] = 5;
    bad(g, "out of range", "src out of range");
    g = chain(5);
    g.dst[1] = -1;
    bad(g, "out of range", "dst negative");
    g = chain(5);
    g.dst[3] = g.src[3];
    bad(g, "to itself", "src == dst");
    g = chain(5);
    g.R[13] = std::numeric_limits<double>::quiet_NaN();
    bad(g, "R not finite", "NaN in R");
    g = chain(5);
    g.t[4] = std::numeric_limits<double>::infinity();
    bad(g, "t not finite", "inf in t");
    g = chain(5);
    g.kappa[0] = 0.0;
    bad(g, "kappa", "kappa == 0");
    g = chain(5);
    g.tau[2] = -1.0;
    bad(g, "tau", "tau < 0");
    g = chain(5);
    g.kappa[1] = std::numeric_limits<double>::quiet_NaN();
    bad(g, "kappa", "kappa NaN");
    g = chain(5);
    g.weight[3] = -0.5;
    bad(g, "weight", "weight < 0");
    g = chain(5);
    g.weight[0] = std::numeric_limits<double>::infinity();
    bad(g, "weight", "weight inf");
    g = chain(5);
    g.n = 0;
    bad(g, "bad argument", "n == 0");
    std::string err;
    const double w[2] = {1.0, std::numeric_limits<double>::quiet_NaN()};
    if (kmx::cert_check_weights(2, w, &err) != KMX_EINVAL || kmx::cert_check_weights(2, nullptr, &err) != KMX_OK) {
      std::fprintf(stderr, "cert_check_weights\n");
      ++g_fail;
    }
  }
  // legal corner cases: no edges, one pose, isolated poses, a hub, parallel and zero-weight edges
  int graphs = 0;
  {
    Graph g;
    g.n = 1;
    check_csr(g, "one pose, no edges");
    g.n = 130;
    check_csr(g, "130 poses, no edges");
    Graph hub;
    hub.n = 300;
    for (int32_t p = 1; p < 201; ++p) (p % 2 ? hub.edge(0, p) : hub.edge(p, 0));
    check_csr(hub, "a hub of 200 incidences and isolated poses");
    Graph par = chain(6);
    par.edge(1, 2);
    par.edge(2, 1);
    par.edge(0, 4, 1.0, 1.0, 0.0);
    par.n = 8;
    check_csr(par, "parallel edges, a zero weight, isolated poses");
    par.with_weight = false;
    check_csr(par, "null weights");
    graphs += 5;
  }
  std::mt19937 rng(4321);
  for (int rep = 0; rep < 200; ++rep) {
    Graph g;
    g.n = 1 + (int32_t)(rng() % 200);
    const int m = (int)(rng() % (3 * g.n));
    for (int k = 0; k < m && g.n > 1; ++k) {
      const int32_t i = rng() % 3 == 0 ? 0 : (int32_t)(rng() % g.n), j = (int32_t)(rng() % g.n);
      if (i != j) g.edge(i, j, 0.5 + (rng() % 7), 0.25 + (rng() % 5), rng() % 5 == 0 ? 0.0 : 1.5);
    }
    check_csr(g, "random graph");
    ++graphs;
  }
  // the start vector: in [-1, 1), the same for the same seed, a prefix of a longer one
  {
    std::vector<double> a(257), b(100);
    kmx::cert_start_vector(7, a.size(), a.data());
    kmx::cert_start_vector(7, b.size(), b.data());
    bool ok = true;
    for (size_t i = 0; i < a.size(); ++i) ok = ok && a[i] >= -1.0 && a[i] < 1.0;
    for (size_t i = 0; i < b.size(); ++i) ok = ok && a[i] == b[i];
    kmx::cert_start_vector(8, b.size(), b.data());
    ok = ok && a[0] != b[0];
    if (!ok) {
      std::fprintf(stderr, "cert_start_vector\n");
      ++g_fail;
    }
  }
  // the tridiagonal solver and the rule against a Jacobi eigensolver
  int decisions[3] = {0, 0, 0}, tri = 0;
  for (int k : {1, 2, 3, 10, 40})
    for (double shift : {-3.0, 0.0, 4.0, 8.0})
      for (int rep = 0; rep < 5; ++rep) {
        const int d = check_tridiag(rng, k, shift);
        if (d >= 0 && d < 3) decisions[d]++;
        ++tri;
      }
  {
    // an invariant subspace: beta[k-1] = 0 certifies a positive tridiagonal and rejects a negative one
    const double a[3] = {2.0, 3.0, 4.0}, b[3] = {0.5, 0.5, 0.0}, an[3] = {-2.0, 3.0, 4.0};
    kmx_cert_result r1, r2, r3;
    std::string err;
    const double nan_b[1] = {std::numeric_limits<double>::quiet_NaN()};
    if (kmx::cert_ritz(3, a, b, 1e-6, &r1, nullptr, &err) != KMX_OK || r1.decision != KMX_CERT_CERTIFIED ||
        r1.residual != 0.0 || kmx::cert_ritz(3, an, b, 1e-6, &r2, nullptr, &err) != KMX_OK ||
        r2.decision != KMX_CERT_NEGATIVE || kmx::cert_ritz(3, a, b, 0.0, &r3, nullptr, &err) != KMX_EINVAL ||
        kmx::cert_ritz(0, a, b, 1.0, &r3, nullptr, &err) != KMX_EINVAL ||
        kmx::cert_ritz(1, a, nan_b, 1.0, &r3, nullptr, &err) != KMX_EINVAL) {
      std::fprintf(stderr, "cert_ritz: invariant subspace / bad arguments\n");
      ++g_fail;
    }
    // the residual factor: one step has s = (1) and rho = beta_1, so eta = 1 certifies up to rho = 1/10
    const double one[1] = {1.0}, b_in[1] = {kmx::CT_RESIDUAL_FACTOR}, b_out[1] = {2.0 * kmx::CT_RESIDUAL_FACTOR};
    const double low[1] = {-0.95};  // theta_min - rho < -eta at rho = 1/10
    if (kmx::cert_ritz(1, one, b_in, 1.0, &r1, nullptr, &err) != KMX_OK || r1.decision != KMX_CERT_CERTIFIED ||
        kmx::cert_ritz(1, one, b_out, 1.0, &r2, nullptr, &err) != KMX_OK || r2.decision != KMX_CERT_UNDECIDED ||
        r2.residual != b_out[0] || kmx::cert_ritz(1, low, b_in, 1.0, &r3, nullptr, &err) != KMX_OK ||
        r3.decision != KMX_CERT_UNDECIDED) {
      std::fprintf(stderr, "cert_ritz: the residual factor\n");
      ++g_fail;
    }
    // the zero matrix (a pose without edges): certified at once
    const double z[1] = {0.0};
    if (kmx::cert_ritz(1, z, z, 1e-9, &r1, nullptr, &err) != KMX_OK || r1.decision != KMX_CERT_CERTIFIED) {
      std::fprintf(stderr, "cert_ritz: zero matrix\n");
      ++g_fail;
    }
  }
  {
    // the scan: the rule is applied at multiples of test_every only, a breakdown ends it at any step
    kmx::CertParams P;
    P.eta = 1e-6;
    P.max_steps = 7;
    P.test_every = 3;
    const double a[7] = {-5.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, b[7] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
    kmx::CertScan sc;
    std::string err;
    int stopped = 0;
    for (int j = 1; j <= 7 && !sc.done; ++j) {
      if (kmx::cert_scan_step(&sc, j, a, b, P, &err) != KMX_OK) ++g_fail;
      stopped = j;
    }
    if (stopped != 3 || sc.res.decision != KMX_CERT_NEGATIVE || sc.res.steps != 3) {
      std::fprintf(stderr, "cert_scan_step: stopped at %d with %d\n", stopped, sc.res.decision);
      ++g_fail;
    }
    const double ap[7] = {5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0}, bb[7] = {1.0, 1.0, 1.0, 1e-20, 1.0, 1.0, 1.0};
    kmx::CertScan s2;
    for (int j = 1; j <= 7 && !s2.done; ++j) {
      if (kmx::cert_scan_step(&s2, j, ap, bb, P, &err) != KMX_OK) ++g_fail;
      stopped = j;
    }
    if (stopped != 4 || !s2.breakdown || s2.res.decision != KMX_CERT_CERTIFIED) {
      std::fprintf(stderr, "cert_scan_step: breakdown at %d with %d\n", stopped, s2.res.decision);
      ++g_fail;
    }
    kmx::CertScan s3;  // max_steps is no test step: undecided, with the values reached
    for (int j = 1; j <= 7 && !s3.done; ++j) {
      if (kmx::cert_scan_step(&s3, j, ap, b, P, &err) != KMX_OK) ++g_fail;
      stopped = j;
    }
    if (stopped != 7 || s3.res.decision != KMX_CERT_UNDECIDED || s3.res.steps != 7) {
      std::fprintf(stderr, "cert_scan_step: max_steps at %d with %d\n", stopped, s3.res.decision);
      ++g_fail;
    }
    kmx_cert_params cp{};
    kmx::CertParams out;
    cp.eta = 0.0;
    int bad_params = kmx::cert_params(&cp, &out, &err) == KMX_EINVAL;
    cp.eta = 1e-5;
    cp.max_steps = -1;
    bad_params += kmx::cert_params(&cp, &out, &err) == KMX_EINVAL;
    cp.max_steps = 0;
    bad_params += kmx::cert_params(nullptr, &out, &err) == KMX_EINVAL;
    if (bad_params != 3 || kmx::cert_params(&cp, &out, &err) != KMX_OK || out.max_steps != 5000 ||
        out.test_every != 10 || out.check_every != 50) {
      std::fprintf(stderr, "cert_params\n");
      ++g_fail;
    }
  }
  {
    // the scan brackets theta_min from the test before: every test must give what the stand-alone rule gives
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const int K = 400;
    std::vector<double> a((size_t)K), b((size_t)K);
    for (int i = 0; i < K; ++i) {
      a[i] = 8.0 + 3.0 * U(rng) - 2.0 * std::exp(-0.05 * i);  // the small end moves, then settles
      b[i] = 0.1 + std::fabs(U(rng));
    }
    kmx::CertParams P;
    P.eta = 1e-300;  // never met: the eigenvectors of a random tridiagonal are localised, rho gets tiny
    P.max_steps = K;
    P.test_every = 10;
    kmx::CertScan sc;
    std::string err;
    int tests = 0;
    for (int j = 1; j <= K && !sc.done; ++j) {
      if (kmx::cert_scan_step(&sc, j, a.data(), b.data(), P, &err) != KMX_OK) ++g_fail;
      if (j % 10 != 0) continue;
      kmx_cert_result ref;
      if (kmx::cert_ritz(j, a.data(), b.data(), P.eta, &ref, nullptr, &err) != KMX_OK) ++g_fail;
      if (std::fabs(ref.theta_min - sc.res.theta_min) > 1e-13 * 16.0 || ref.decision != sc.res.decision ||
          std::fabs(ref.residual - sc.res.residual) > 1e-9) {
        std::fprintf(stderr, "scan at %d: theta_min %.17g vs %.17g, rho %.3e vs %.3e\n", j, sc.res.theta_min,
                     ref.theta_min, sc.res.residual, ref.residual);
        ++g_fail;
      }
      ++tests;
    }
    if (tests != K / 10) {
      std::fprintf(stderr, "scan: %d tests\n", tests);
      ++g_fail;
    }
  }
  if (decisions[KMX_CERT_UNDECIDED] == 0 || decisions[KMX_CERT_CERTIFIED] == 0 || decisions[KMX_CERT_NEGATIVE] == 0) {
    std::fprintf(stderr, "tridiagonal cases did not reach each of the three decisions\n");
    ++g_fail;
  }
  if (g_fail) {
    std::fprintf(stderr, "cert_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("cert_check ok: %d graphs with their CSR verified, %d malformed graphs refused, %d tridiagonals "
              "(undecided %d, certified %d, negative %d)\n",
              graphs, refused, tri, decisions[0], decisions[1], decisions[2]);
  return 0;
}
